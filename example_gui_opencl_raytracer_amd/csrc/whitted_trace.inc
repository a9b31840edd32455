/*
 * whitted_trace.inc -- the per-pixel Whitted trace for CDNA4 (gfx950), hand-written HIP.
 *
 * Included by whitted_fast.hip and whitted_strict.hip, which define WT_STRICT and the
 * namespace.  What it computes is the reference's `raygen` + `raytracer` kernels
 * (reference src/cl/raygen.cl:5-25, raytracing.cl:14-195, primitives.cl:14-442); how it
 * computes it is CDNA4-first:
 *
 *   - one 64-lane wavefront owns one 8x8 pixel tile and is its own workgroup; tile rows are
 *     dealt to the 8 XCDs round-robin so every framebuffer cache line is written by exactly
 *     one XCD's L2;
 *   - primary rays are generated in registers (the 64 B/pixel ray buffer never touches HBM
 *     in the fused mode);
 *   - the scene is a prepared 16-B-per-primitive float4 stream staged once per workgroup
 *     in LDS and read with wave-uniform (broadcast) ds_read_b128; materials are gathered
 *     only for the winning primitive;
 *   - the reference's 15-deep private ray stack (1 088 B of scratch per lane) becomes a
 *     12-word parent record per DFS level: the first WT_LDS_LEVELS levels live in LDS
 *     ([level][word][lane], conflict-free), deeper levels (depth > 4 only) in scratch;
 *   - the six shadow rays of a hit are traced together by their lane (shared origin-only halves, six
 *     independent chains); the loops are wave-uniform with ballot early-outs: the wave stops testing
 *     primitives as soon as every live ray is decided, skips the root half of a sphere no lane's line
 *     meets, and skips the shadow rays of surfaces whose Phong coefficients are zero;
 *   - each XCD's tiles are served heaviest-first from the previous frame's per-tile cost (wt_sched_build);
 *   - scenes with many spheres walk a uniform grid (wt_grid_*), same arithmetic per test;
 *   - deep launches (depth > 4) hand the tail of a tile -- the refraction trees of its last live lanes -- to the tree-parallel tail
 *     (whitted_tpt.inc): pending paths become a pool of nodes traced 64 at a time by the whole wave, shaded by the same six-ray batch,
 *     added up per pixel in the reference's order; heavy tiles are served by several wavefronts (wt_sched_build);
 *   - no MFMA: there is no dense contraction on this path; no packed fp32 (no gain on gfx950).
 *
 * Semantics kept bug-for-bug (SURVEY.md Appendix B): see the comments at each step.
 */

#ifndef WT_STRICT
#error "WT_STRICT must be defined (0: fast, 1: strict)"
#endif

#define WT_EPSILON 0.001f            /* primitives.cl:5  */
#define WT_THROUGH 0.8f              /* primitives.cl:7: the default of whitted_params.through */
#define WT_DEFAULT_N 1.0f            /* raytracing.cl:7  */
#define WT_SOFT 2                    /* raytracing.cl:10 */
/* Parent records per wave: 12 words x 64 lanes = 3 KB per DFS level.  How many levels live in LDS sets how many waves
 * a CU can hold (160 KB of LDS), and with the registers capped to match, the occupancy:
 *   fast, depth <= 4 (three levels needed): 2 in LDS + 1 in scratch, registers capped for 5 waves/SIMD (96 VGPRs, a
 *     few spills): -8.5 % kernel time against 3 levels in LDS at 4.25 waves/SIMD -- these launches are throughput
 *     bound, and the third level is touched by few pixels;
 *   deep (depth > 4), two flavours picked per launch by the shim: 3 LDS levels / uncapped registers for launches whose
 *     time is the serial chain of their deepest refraction trees (800x600 and 1920x1080 at depth 15: the capped flavour
 *     is 2-3 % slower there), 2 LDS levels / 5 waves (WT_F_OCC) for launches of >= 9 000 x depth tiles (4096^2 depth 8: -13 %);
 *   strict: 3 levels in LDS, uncapped (its libm calls spill under the cap: +1 %). */
#ifndef WT_LDS_LEVELS
#if WT_STRICT
#define WT_LDS_LEVELS 3              /* parent records kept in LDS by the shallow build (depth <= 4 needs 3) */
#else
#define WT_LDS_LEVELS 2
#endif
#endif
#ifndef WT_LDS_LEVELS_DEEP
#define WT_LDS_LEVELS_DEEP 3         /* the same for the deep build (depth > 4)           */
#endif
#ifndef WT_LDS_LEVELS_DEEP_OCC
#define WT_LDS_LEVELS_DEEP_OCC 1     /* ... and for its high-occupancy flavour: with two levels the LDS, not the 96-VGPR cap, set the
                                      * residency (18 of 20 waves per CU; C3 8.17 -> 7.77 ms with one; depth 15: +1 %) */
#endif
#ifndef WT_MIN_WAVES
#define WT_MIN_WAVES (WT_STRICT ? 2 : 3)   /* __launch_bounds__ waves per SIMD of the deep build's low-occupancy flavour: 168 VGPRs (it sat at 166-177 without a cap; the
                                      * tail's expansion pass would take it to 193 = two waves); strict: 256 */
#endif
#ifndef WT_OCC_WAVES
#define WT_OCC_WAVES 5
#endif
#ifndef WT_GRID_SHALLOW_WAVES
#define WT_GRID_SHALLOW_WAVES WT_OCC_WAVES   /* fast grid build, depth <= 4 */
#endif
#ifndef WT_SHALLOW_WAVES
#if WT_STRICT
#define WT_SHALLOW_WAVES 4           /* 128 VGPRs: the strict build sits at 128-131 registers uncapped, and 131 would cost a whole wave per SIMD */
#else
#define WT_SHALLOW_WAVES WT_OCC_WAVES
#endif
#endif
#define WT_REC 12                    /* words per parent record                           */
#ifndef WT_TPT_RC
#define WT_TPT_RC 8                   /* positions the tail's replay requests per round (fast build; 4: ref800 +3 %, 1920x1080 depth 15 +2.6 %) */
#endif
#ifndef WT_TPT_RSTK_LDS           /* A/B switches of the tree-parallel tail (whitted_tpt.inc) */
#define WT_TPT_RSTK_LDS 1
#endif
#ifndef WT_TPT_FORWARD
#define WT_TPT_FORWARD 1
#endif
#ifndef WT_CULL_MIN_SPHERES
#define WT_CULL_MIN_SPHERES 16u         /* deep builds: from this many spheres on a wave's shadow batch first asks which spheres its rays can meet (wt_sphere_candidates) */
#endif
#define WT_TPT_MAX_BATCHES 1022      /* batches of <= 64 nodes the tree-parallel tail can hold (whitted_tpt.inc) */

/* ---- in-kernel stamps (DIAGNOSTIC build only: -DWT_STAMPS=1, library tag _stamp, tools/stamp_phases.py) ------------
 * s_memtime at the phase boundaries of the per-lane loop, differences summed per phase in scalar registers and added
 * to words 16.. of the counter block at the end of the wave.  Wave-level time: a scalar instruction executes once per
 * wave whichever lanes are active.  Never compiled into the product (in the real kernel no stamp executes); read the
 * SHARES, not the run time of this build. */
enum { WT_ST_LOOP = 0, WT_ST_PROBE = 1, WT_ST_NEAREST = 2, WT_ST_RESOLVE = 3, WT_ST_LIGHTS = 4, WT_ST_SHADOW = 5,
       WT_ST_ADD = 6, WT_ST_BOUNCE = 7, WT_ST_POP = 8, WT_ST_PROLOG = 9, WT_ST_N = 10 };
#ifdef WT_STAMPS
/* state in LDS, updated by the first ACTIVE lane: registers would become per-lane values under the divergent control
 * flow the stamps sit in (each lane would only see the stamps it executed itself) */
#define WT_STAMP_DECL __shared__ unsigned s_st[WT_ST_N + 2]; \
    if (threadIdx.x == 0) { for (int k_ = 0; k_ < WT_ST_N; k_++) s_st[k_] = 0u; s_st[WT_ST_N] = (unsigned)wt_stamp_now(); } \
    __syncthreads();
#define WT_STAMP(k) do { __builtin_amdgcn_sched_barrier(0); const unsigned t_ = (unsigned)wt_stamp_now(); \
                         if ((threadIdx.x & 63u) == (unsigned)__builtin_ctzll(__builtin_amdgcn_ballot_w64(true))) { \
                             s_st[k] += t_ - s_st[WT_ST_N]; s_st[WT_ST_N] = t_; } \
                         __builtin_amdgcn_sched_barrier(0); } while (0)
__device__ __forceinline__ unsigned long long wt_stamp_now() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    return t;
}
#else
#define WT_STAMP_DECL
#define WT_STAMP(k) do { } while (0)
#endif

/* (Measured on MI355X and removed again, numbers in profiles/r02_ab_experiments.txt: materials / texture rows of a small scene in LDS,
 * the skybox texel of a miss or the ambient term deferred past the shade block, a wave-wide pool of shadow rays and paired
 * soft-shadow walks for the grid builds, a persistent tile-pulling launch.) */
#ifndef WT_TIMELINE
#define WT_TIMELINE 0        /* DIAGNOSTIC: see whitted_params.h `diag` */
#endif
#ifndef WT_COST_LIFETIME
#define WT_COST_LIFETIME 0   /* DIAGNOSTIC: every build books a tile's wave lifetime as its cost (tools/tile_costs.py) */
#endif

template <int N> struct wt_int { static constexpr int value = N; };      /* a compile-time count handed to a generic lambda */
struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk3(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 operator*(f3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
/* Both builds are compiled with -ffp-contract=off.  The fast build fuses exactly where it is written here, so
 * its arithmetic does not depend on compiler heuristics or on which copy of an inlined helper a segment runs
 * through (the image must not depend on how pixels are grouped into waves). */
#if WT_STRICT
__device__ __forceinline__ float dot3(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float wt_fma(float a, float b, float c) { return a * b + c; }
#else
__device__ __forceinline__ float dot3(f3 a, f3 b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ float wt_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
#endif
/* a * s + b */
__device__ __forceinline__ f3 wt_madd3(f3 a, float s, f3 b);
__device__ __forceinline__ f3 wt_madd3(f3 a, float s, f3 b) {
    return mk3(wt_fma(a.x, s, b.x), wt_fma(a.y, s, b.y), wt_fma(a.z, s, b.z));
}

/* ---- the two arithmetic modes ------------------------------------------------------ */
#if WT_STRICT
__device__ __forceinline__ float wt_div(float a, float b) { return a / b; }   /* IEEE */
__device__ __forceinline__ float wt_sqrt(float a) { return sqrtf(a); }         /* IEEE */
__device__ __forceinline__ f3 wt_scale_inv(f3 v, float len) { return mk3(v.x / len, v.y / len, v.z / len); }
#else
/* v_rcp_f32 / v_sqrt_f32 are 1 ulp: inside OpenCL's 2.5 / 3 ulp bounds for x/y and sqrt */
__device__ __forceinline__ float wt_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ float wt_sqrt(float a) { return __builtin_amdgcn_sqrtf(a); }
__device__ __forceinline__ f3 wt_scale_inv(f3 v, float len) { return v * __builtin_amdgcn_rcpf(len); }
#endif

/* sin/cos of the light-sampling angles and the Blinn-Phong pow (base in [0,1], exponent = (float)uint
 * shininess, raytracing.cl:129).
 * The angles are theta = fl32(2*pi * u1), phi = fl32(pi * u2) with u in [0,4) and the product taken in fp64
 * (M_PI is a double constant, raytracing.cl:99-100); wt_sincos_angle<FULL>(u) returns sin/cos of that fp32 angle.
 * strict: the fp64 product, then the device libm (ocml), which agrees with the oracle's glibc on every value tested.
 * fast:   the hardware v_sin_f32 / v_cos_f32 take REVOLUTIONS, and u (or u/2) IS the angle in revolutions, exactly:
 *         no fp64 product, no range reduction, two instructions.  Against the reference's sin/cos of the ROUNDED
 *         angle this differs by that rounding (<= 0.95e-6 rad at 8 pi) plus the hardware's error (1.25e-7 absolute,
 *         tools/ubench/hw_trig.hip): <= 1.2e-6 absolute, i.e. the sample point on the radius-0.1 light moves by
 *         <= 1.2e-7 and the shadow ray turns by less than an fp32 direction can resolve.  A shadow ray's outcome is
 *         binary (raytracing.cl:111-115), so only a ray grazing a silhouette that closely can change; measured:
 *         images unchanged.
 *         pow = exp2(y * log2 x) on the hardware v_log_f32 / v_exp_f32, with a compensated series for x > 2/3
 *         where v_log_f32 loses relative accuracy (host model: <= 6 ulp; OpenCL allows 16). */
#if WT_STRICT
template <bool FULL>
__device__ __forceinline__ void wt_sincos_angle(float u, float& sn, float& cs) {
    const float x = (float)((FULL ? 2 * 3.14159265358979323846 : 3.14159265358979323846) * (double)u);
    sincosf(x, &sn, &cs);
}
__device__ __forceinline__ float wt_pow(float x, float y) { return powf(x, y); }
#else
template <bool FULL>
__device__ __forceinline__ void wt_sincos_angle(float u, float& sn, float& cs) {
    const float rev = FULL ? u : 0.5f * u;
    sn = __builtin_amdgcn_sinf(rev);
    cs = __builtin_amdgcn_cosf(rev);
}
__device__ __forceinline__ float wt_pow(float x, float y) {
    /* log2 x as a two-float sum for x > 2/3 (2 atanh-series of s = (x-1)/(x+1), compensated), hardware v_log_f32
     * below; y * log2 x with its rounding error carried; exp2 on the hardware.  Host model: <= 6 ulp for results
     * >= 2^-10, absolute error <= 7e-8 on [0,1] for y up to 1000 (OpenCL allows 16 ulp). */
    const bool near1 = x > 0.6666667f;
    float L_hi = 0.0f, L_lo = 0.0f;
    if (__builtin_amdgcn_ballot_w64(near1) != 0) {              /* the series only when some lane needs it */
        const float t = x - 1.0f;                               /* exact for x in [0.5, 2] */
        const float den = 2.0f + t;
        const float rc = __builtin_amdgcn_rcpf(den);
        float s = t * rc;
        s = __builtin_fmaf(__builtin_fmaf(-s, den, t), rc, s);  /* one Newton step */
        const float s_lo = __builtin_fmaf(-s, den, t) * rc;
        const float s2 = s * s;
        const float P = s2 * __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(0.1111111111f, s2, 0.1428571429f), s2, 0.2f), s2, 0.3333333333f);
        const float ch = 2.8853900432586669921875f, cl = 3.851925025061160e-08f;   /* 2 / ln 2 = ch + cl */
        const float ph = ch * s;
        const float pl = __builtin_fmaf(ch, s, -ph) + __builtin_fmaf(cl, s, ch * s_lo);
        const float corr = __builtin_fmaf(ph, P, pl);
        L_hi = ph + corr;
        L_lo = (ph - L_hi) + corr;                              /* fast two-sum */
    }
    if (!near1) { L_hi = __builtin_amdgcn_logf(x); L_lo = 0.0f; }   /* v_log_f32 = log2 */
    const float yh = y * L_hi;
    const float yl = __builtin_fmaf(y, L_hi, -yh) + y * L_lo;
    const float r = __builtin_amdgcn_exp2f(yh);
    const float res = __builtin_fmaf(r * 0.69314718056f, yl, r);
    return (y == 0.0f) ? 1.0f : ((x == 0.0f) ? 0.0f : res);
}
#endif

/* normalize(v) and |v| together: OpenCL normalize = v / sqrt(dot(v,v)) */
__device__ __forceinline__ f3 wt_normalize_len(f3 v, float& len) {
#if !WT_STRICT   /* one v_rsq_f32 (1 ulp) instead of v_sqrt_f32 + v_rcp_f32: |v| = d2 * rsq(d2) */
    const float d2 = dot3(v, v);
    const float rs = __builtin_amdgcn_rsqf(d2);
    len = d2 * rs;
    return v * rs;
#else
    len = wt_sqrt(dot3(v, v));
    return wt_scale_inv(v, len);
#endif
}
__device__ __forceinline__ f3 wt_normalize(f3 v) { float l; return wt_normalize_len(v, l); }

/* raygen.cl:13-21, identical in both arithmetic modes (no contraction, IEEE sqrt/divide): it
 * runs once per pixel, and primary rays that graze the floor near the horizon amplify a
 * 1-ulp direction change into a different checker texel, so this is kept bit-exact. */
__device__ __forceinline__ f3 wt_primary_dir_xy(const float* corner, const float* right, const float* up,
                                                float w_factor, float h_factor, unsigned px, unsigned py);
__device__ __forceinline__ f3 wt_primary_dir(const float* corner, const float* right, const float* up,
                                             float w_factor, float h_factor, unsigned id32, unsigned width) {
    return wt_primary_dir_xy(corner, right, up, w_factor, h_factor, id32 % width, id32 / width);
}
/* the same from the pixel's column and row (id % W, id / W of raygen.cl:13-14): the tiled mapping knows them */
__device__ __forceinline__ f3 wt_primary_dir_xy(const float* corner, const float* right, const float* up,
                                                float w_factor, float h_factor, unsigned px, unsigned py) {
#pragma clang fp contract(off)
    const float w = (float)px;
    const float h = (float)py;
    float vx = corner[0] + right[0] * w_factor * w - up[0] * h_factor * h;
    float vy = corner[1] + right[1] * w_factor * w - up[1] * h_factor * h;
    float vz = corner[2] + right[2] * w_factor * w - up[2] * h_factor * h;
    float len = sqrtf(vx * vx + vy * vy + vz * vz);
    return mk3(vx / len, vy / len, vz / len);
}
/* the same with a camera of the lane's own (the sample cameras of a supersampled launch): the same operations in the same order */
__device__ __forceinline__ f3 wt_primary_dir_xy(f3 corner, f3 right, f3 up, float w_factor, float h_factor, unsigned px, unsigned py) {
#pragma clang fp contract(off)
    const float w = (float)px;
    const float h = (float)py;
    float vx = corner.x + right.x * w_factor * w - up.x * h_factor * h;
    float vy = corner.y + right.y * w_factor * w - up.y * h_factor * h;
    float vz = corner.z + right.z * w_factor * w - up.z * h_factor * h;
    float len = sqrtf(vx * vx + vy * vy + vz * vz);
    return mk3(vx / len, vy / len, vz / len);
}

/* (int)f as AMD hardware converts it: saturating, NaN -> 0 (v_cvt_i32_f32) */
__device__ __forceinline__ int wt_f2i(float f) { return (int)f; }

__device__ __forceinline__ int wt_emod(int a, int b) { /* primitives.cl:162-168 */
    int m = a % b;
    if (m < 0) m = (b < 0) ? m - b : m + b;
    return m;
}

/* primitives.cl:116-125: returns [0,4) -- (float)x / 2^31 * 2 is an exact scaling by 2^-30 */
__device__ __forceinline__ float wt_xorshift(unsigned& s) {
    unsigned x = s;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    s = x;
    return (float)x * 9.31322574615478515625e-10f;   /* 2^-30: both scalings are by powers of two, so one multiply is the same value */
}

/* Per-ray invariants of intersect_sphere (primitives.cl:173,181,188): a = d.d, 4a, 2a */
struct rayq {
    f3 o, d;
    float a4;   /* a = d.d          (the names date from the reference's 4ac / 2a; see wt_sphere_pre: the test runs on b/2 and D/4) */
    float a2;   /* a (strict) or 1/a (fast) */
};
/* unit_rt (wave-uniform): the direction is known to be normalised -- fast build, rays generated by this library (primary rays
 * are normalised by raygen, fused or as its own kernel; reflect / refract preserve the length to rounding): a = d.d =
 * 1 +- a few 1e-7 is taken as exactly 1, as for the shadow rays below -- no dot product, no v_rcp_f32, and the factors 4a
 * and 1/(2a) become constants.  Moves a hit distance by <= 2e-7 relative.  Rays uploaded by a caller keep the full
 * quadratic, and so do big scenes (more than 256 spheres, grid or not: there b*b and 4ac agree to 5-7 digits, so 3e-7
 * is not below the noise -- it moved 1.4 % of C4's pixels). */
template <bool UNIT>
__device__ __forceinline__ rayq wt_rayq(f3 o, f3 d, bool unit_rt = false) {
    rayq r; r.o = o; r.d = d;
#if !WT_STRICT
    if (UNIT || unit_rt) { r.a4 = 1.0f; r.a2 = 1.0f; return r; }
#endif
    float a = dot3(d, d);
    r.a4 = a;
#if WT_STRICT
    r.a2 = a;
#else
    r.a2 = __builtin_amdgcn_rcpf(a);
#endif
    return r;
}

/* primitives.cl:170-195.  s = {cx,cy,cz,+-r^2}.  The test is split in two so that rays sharing an
 * origin (the six shadow rays of one hit) share v = o - c, 2v and c = v.v - r^2: the same values the
 * reference recomputes per test.  NaN behaviour of the comparisons is kept: `D < 0` and `t2 <= 0`
 * are the rejecting tests. */
/* The reference's b = dot(2v, d), D = b^2 - 4ac, t = (-b -+ sqrt D) / 2a are evaluated as b/2 = v.d, D/4 = (b/2)^2 - ac,
 * t = (-b/2 -+ sqrt(D/4)) / a: every factor of two is an exact scaling, it commutes with each rounding (and with v_rcp_f32), so
 * b/2, D/4 and sqrt(D/4) are exactly half, a quarter and half of the reference's values, the comparisons `D < 0`, `t <= 0`
 * see the same signs and t has the same bits (below 1e-19 an underflow could differ; no ray gets there) -- three multiplies
 * less per test in both builds. */
struct sph_pre { f3 v2; float c; };     /* v2 = v = o - centre (the name dates from 2v) */
__device__ __forceinline__ sph_pre wt_sphere_pre(f3 o, float4 s) {
    sph_pre p;
    p.v2 = o - mk3(s.x, s.y, s.z);
    p.c = dot3(p.v2, p.v2) - fabsf(s.w);
    return p;
}
/* discriminant half (b, D) and root half (t) of the test: a wave skips the root half of a primitive
 * when no lane has D >= 0 -- most rays miss most spheres */
__device__ __forceinline__ bool wt_sphere_disc(const sph_pre& p, f3 d, float a4, float& b, float& D) {
    b = dot3(p.v2, d);
    D = wt_fma(b, b, -(a4 * p.c));
    return !(D < 0);
}
__device__ __forceinline__ bool wt_sphere_root(float b, float D, float a2, float& t) {
    float sD = wt_sqrt(D);
#if WT_STRICT
    float t0 = (-b - sD) / a2;
    float t2 = (t0 < 0) ? (-b + sD) / a2 : t0;
#else
    float t0 = (-b - sD) * a2;
    float t2 = (t0 < 0) ? (-b + sD) * a2 : t0;
#endif
    t = t2;
    return !(t2 <= 0);
}
__device__ __forceinline__ bool wt_sphere_dir(const sph_pre& p, f3 d, float a4, float a2, float& t) {
    float b, D;
    bool ok = wt_sphere_disc(p, d, a4, b, D);
    return wt_sphere_root(b, D, a2, t) && ok;
}
/* single-ray form used by the light probe and the nearest-hit search: wave-level skip of the root half */
__device__ __forceinline__ bool wt_sphere(const rayq& r, float4 s, float& t) {
    const sph_pre p = wt_sphere_pre(r.o, s);
    float b, D;
    const bool ok = wt_sphere_disc(p, r.d, r.a4, b, D);
    bool hit = false;
    t = 0.0f;
    if (__builtin_amdgcn_ballot_w64(ok)) hit = wt_sphere_root(b, D, r.a2, t) && ok;
    return hit;
}

/* ---- the same test for SHADOW rays --------------------------------------------------------------------
 * strict: exactly the functions above.
 * fast:   a shadow ray's direction has just been normalised, so a = d.d = 1 +- 3e-7 is taken as exactly 1.  With
 *         4a = 4 and 1/(2a) = 1/2 every factor of two drops out exactly -- b/2 = v.d, D/4 = (v.d)^2 - c,
 *         t = -b/2 -+ sqrt(D/4) -- so no per-ray invariants are kept at all (12 registers and a v_rcp_f32 per
 *         ray less).  The outcome of a shadow ray is binary (blocked or not, raytracing.cl:111-115), so taking
 *         a = 1 can only move rays that graze a silhouette within ~1e-7; measured: images unchanged. */
#if WT_STRICT
__device__ __forceinline__ rayq wt_shadow_rayq(f3 o, f3 d) { return wt_rayq<false>(o, d); }
__device__ __forceinline__ sph_pre wt_shadow_pre(f3 o, float4 s) { return wt_sphere_pre(o, s); }
__device__ __forceinline__ bool wt_shadow_disc(const sph_pre& p, f3 d, float a4, float& b, float& D) { return wt_sphere_disc(p, d, a4, b, D); }
__device__ __forceinline__ bool wt_shadow_root(float b, float D, float a2, float& t) { return wt_sphere_root(b, D, a2, t); }
#else
__device__ __forceinline__ rayq wt_shadow_rayq(f3 o, f3 d) { rayq r; r.o = o; r.d = d; r.a4 = 1.0f; r.a2 = 1.0f; return r; }
__device__ __forceinline__ sph_pre wt_shadow_pre(f3 o, float4 s) {   /* v2 holds v itself here */
    sph_pre p;
    p.v2 = o - mk3(s.x, s.y, s.z);
    p.c = dot3(p.v2, p.v2) - fabsf(s.w);
    return p;
}
__device__ __forceinline__ bool wt_shadow_disc(const sph_pre& p, f3 d, float, float& b, float& D) {
    b = dot3(p.v2, d);
    D = __builtin_fmaf(b, b, -p.c);
    return !(D < 0);
}
__device__ __forceinline__ bool wt_shadow_root(float b, float D, float, float& t) {
    const float sD = wt_sqrt(D);
    const float t0 = -b - sD;
    t = (t0 < 0) ? (-b + sD) : t0;
    return !(t <= 0);
}
#endif
__device__ __forceinline__ bool wt_shadow_dir(const sph_pre& p, f3 d, float a4, float a2, float& t) {
    float b, D;
    bool ok = wt_shadow_disc(p, d, a4, b, D);
    return wt_shadow_root(b, D, a2, t) && ok;
}
/* Which form a launch's shadow rays take is a property of the SCENE, so that every way of tracing it (LDS or global geometry, grid
 * walk or linear scan) computes the same bits: a = 1 in small scenes, the full quadratic in big ones (more than 256 spheres: rays
 * start up to a hundred units from the spheres they pass, b*b and 4ac agree to 5-7 digits and 3e-7 of a is not below that noise).
 * LDS-geometry kernels only ever see small scenes and use the a = 1 forms above; the others take a4 / a2 from here and run the
 * general wt_sphere_disc / wt_sphere_root, which with a4 = a2 = 1 give exactly the a = 1 forms' values (x1 is exact). */
#define WT_BIG_SCENE_SPHERES 256u    /* = GRID_MIN_SPHERES of hip_wrap.cpp */
template <bool GEOM_LDS>
__device__ __forceinline__ rayq wt_shadow_rayq_scene(const whitted_params& P, f3 o, f3 d) {
    if (GEOM_LDS || P.ns <= WT_BIG_SCENE_SPHERES) return wt_shadow_rayq(o, d);
    return wt_rayq<false>(o, d);
}
template <bool GEOM_LDS>
__device__ __forceinline__ bool wt_shadow_disc_g(const sph_pre& p, f3 d, float a4, float& b, float& D) {
    return GEOM_LDS ? wt_shadow_disc(p, d, a4, b, D) : wt_sphere_disc(p, d, a4, b, D);
}
template <bool GEOM_LDS>
__device__ __forceinline__ bool wt_shadow_root_g(float b, float D, float a2, float& t) {
    return GEOM_LDS ? wt_shadow_root(b, D, a2, t) : wt_sphere_root(b, D, a2, t);
}

/* primitives.cl:197-215, split the same way: num = (p0 - o).n depends on the origin only */
__device__ __forceinline__ float wt_plane_pre(f3 o, float4 n, float4 p0) {
    return dot3(mk3(p0.x, p0.y, p0.z) - o, mk3(n.x, n.y, n.z));
}
__device__ __forceinline__ bool wt_plane_dir(float num, float4 n, f3 d, float& t) {
    float b = dot3(d, mk3(n.x, n.y, n.z));
    float t2 = wt_div(num, b);
    t = t2;
    return !(b == 0) && !(t2 <= 0);
}
/* shadow rays only need "is the plane hit in front of the light sample": hit && !(t >= tl) of
 * testShadowPath (primitives.cl:422-437).  strict: through the divide, as written there.  fast: the same
 * predicate without the divide -- t > 0 <=> num*b > 0, t < tl <=> |num| < tl*|b| -- with the comparisons negated
 * the same way so a NaN ray is still "blocked". */
__device__ __forceinline__ bool wt_plane_blocks(float num, float4 n, f3 d, float tl) {
#if WT_STRICT
    float t;
    const bool hit = wt_plane_dir(num, n, d, t);
    return hit && !(t >= tl);
#else
    const float b = dot3(d, mk3(n.x, n.y, n.z));
    return !(num * b <= 0) && !(fabsf(num) >= tl * fabsf(b));
#endif
}
__device__ __forceinline__ bool wt_plane(const rayq& r, float4 n, float4 p0, float& t) {
    return wt_plane_dir(wt_plane_pre(r.o, n, p0), n, r.d, t);
}

/* ---- material fields of the raw 64-B rmaterial (types.cl:4-19) at byte offset 32 of a
 *      96-B rsphere / rplane ---------------------------------------------------------- */
struct mat_t {
    f3 rgb;
    float ambient, diffuse, specular, shininess;
    unsigned transparent, dielectric;
    float n, reflectivity;
};
/* float4 k (0: rgb | 1: ambient, diffuse, specular, shininess | 2: transparent, dielectric, n, reflectivity) of the
 * material of primitive `prim` (sphere index, or ns + plane index), gathered from the raw arrays for the winner only. */
__device__ __forceinline__ float4 wt_mat_f4(const whitted_params& P, unsigned prim, unsigned k, unsigned ns) {   /* ns = P.ns */
    const uint8_t* raw = prim < ns ? P.spheres_raw + 96 * (size_t)prim : P.planes_raw + 96 * (size_t)(prim - ns);
    return ((const float4*)(raw + 32))[k];
}
__device__ __forceinline__ void wt_mat_set_b(mat_t& m, float4 b) {
    m.ambient = b.x; m.diffuse = b.y; m.specular = b.z;
    m.shininess = (float)__float_as_uint(b.w);
}
__device__ __forceinline__ void wt_mat_set_c(mat_t& m, float4 c) {
    m.transparent = __float_as_uint(c.x);
    m.dielectric = __float_as_uint(c.y);
    m.n = c.z; m.reflectivity = c.w;
}

/* (float)byte / 255.0f, correctly rounded in both modes: a texel colour times a simple factor often
 * lands within an ulp of an integer after the final *255, so a 1-ulp error here would flip the
 * truncating 8-bit pack over whole regions.  fast: one FMA residual step on x * (1/255), exact for
 * all 256 inputs (checked exhaustively); strict: IEEE divide. */
__device__ __forceinline__ float wt_unorm8(unsigned b) {
    const float x = (float)b;
#if WT_STRICT
    return x / 255.0f;
#else
    const float r255 = 1.0f / 255.0f;
    const float q = x * r255;
    return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, x), r255, q);
#endif
}
__device__ __forceinline__ f3 wt_texel_rgb(unsigned px) {
    return mk3(wt_unorm8(px & 255u), wt_unorm8((px >> 8) & 255u), wt_unorm8((px >> 16) & 255u));
}

/* primitives.cl:14-109 map_to_cube + the fetch of raytracing.cl:61-77.  Six independent
 * ifs, later faces win ties; v is flipped as height - v.  Coordinates outside the image
 * (undefined in OpenCL) are clamped to the edge. */
/* the (u, v) of map_to_cube (primitives.cl:14-109) for a cross of face size `face` */
__device__ __forceinline__ void wt_cube_uv(f3 dir, unsigned face, int& u, int& v) {
    float x = dir.x, y = dir.y, z = dir.z;
    float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
    const bool xp = x > 0, yp = y > 0, zp = z > 0;
    /* the reference's six independent ifs, later faces winning ties (z over y over x), as selects: a direction
     * with a NaN component matches no face and keeps maxa = uc = vc = 0 (-> 0/0), as there */
    const bool xmaj = ax >= ay && ax >= az, ymaj = ay >= ax && ay >= az, zmaj = az >= ax && az >= ay;
    const float maxa = zmaj ? az : (ymaj ? ay : (xmaj ? ax : 0.0f));
    const float uc = zmaj ? (zp ? x : -x) : (ymaj ? x : (xmaj ? (xp ? -z : z) : 0.0f));
    const float vc = zmaj ? y : (ymaj ? (yp ? -z : z) : (xmaj ? y : 0.0f));
    const unsigned su = zmaj ? (zp ? face : face * 3) : (ymaj ? face : (xmaj ? (xp ? face * 2 : 0u) : 0u));
    const unsigned sv = zmaj ? face : (ymaj ? (yp ? face * 2 : 0u) : (xmaj ? face : 0u));
    float fu = 0.5f * (wt_div(uc, maxa) + 1.0f);
    float fv = 0.5f * (wt_div(vc, maxa) + 1.0f);
    u = wt_f2i((float)su + fu * (float)face);
    v = wt_f2i((float)sv + fv * (float)face);
}
__device__ __forceinline__ unsigned wt_skybox_fetch(const whitted_params& P, f3 dir) {
    int u, vv;
    wt_cube_uv(dir, (unsigned)(P.sky_w / 4), u, vv);
    int v = P.sky_h - vv;
    u = min(max(u, 0), P.sky_w - 1);
    v = min(max(v, 0), P.sky_h - 1);
    return P.sky[(size_t)v * (size_t)P.sky_w + (size_t)u];
}

/* primitives.cl:217-259 with the per-plane tangent basis hoisted to scene preparation */
/* Returns the texel WORD; wt_texel_rgb converts it where the colour is used (the ambient term, after the shadow rays). */
__device__ __forceinline__ unsigned wt_plane_texel_fetch(const whitted_params& P, unsigned plane, f3 p) {
    const float4* pt = (const float4*)P.ptex + 2 * plane;
    const float4 b0 = pt[0], b1 = pt[1];
    float ui = dot3(mk3(b0.x, b0.y, b0.z), p) * b0.w;
    float vi = dot3(mk3(b1.x, b1.y, b1.z), p) * b0.w;
    int tx, ty;
    /* euclidean_modulo (primitives.cl:162-168) by a power of two is a mask, also for negative coordinates
     * (two's complement); wave-uniform choice, the general form costs two integer divisions per fetch */
    if ((((unsigned)P.tex_w & ((unsigned)P.tex_w - 1u)) | ((unsigned)P.tex_h & ((unsigned)P.tex_h - 1u))) == 0u) {
        tx = wt_f2i(ui) & (P.tex_w - 1);
        ty = wt_f2i(vi) & (P.tex_h - 1);
    } else {
        tx = wt_emod(wt_f2i(ui), P.tex_w);
        ty = wt_emod(wt_f2i(vi), P.tex_h);
    }
    int layer = min(max(__float_as_int(b1.w), 0), P.tex_layers - 1);
    return P.tex[((size_t)layer * (size_t)P.tex_h + (size_t)ty) * (size_t)P.tex_w + (size_t)tx];
}

/* primitives.cl:127-130 / 132-144 / 146-160 */
__device__ __forceinline__ f3 wt_reflect(f3 i, f3 n) {
    float cosI = -dot3(n, i);
    return wt_madd3(n, 2 * cosI, i);
}
__device__ __forceinline__ bool wt_refract(float n1, float n2, f3 i, f3 nrm, f3& out) {
    float n = wt_div(n1, n2);
    float cosI = -dot3(nrm, i);
    float sinT2 = n * n * (1.0f - cosI * cosI);
    if (sinT2 > 1.0f) return false; /* reference returns a NaN vector; caller drops the child */
    float cosT = wt_sqrt(1.0f - sinT2);
    out = wt_madd3(nrm, n * cosI - cosT, i * n);
    return !(out.x != out.x);
}
__device__ __forceinline__ float wt_schlick(float n1, float n2, f3 i, f3 nrm) {
    float r0 = wt_div(n1 - n2, n1 + n2);
    r0 *= r0;
    float cosX = -dot3(nrm, i);
    if (n1 > n2) {
        float n = wt_div(n1, n2);
        float sinT2 = n * n * (1.0f - cosX * cosX);
        if (sinT2 > 1.0f) return 1.0f;
        cosX = wt_sqrt(1.0f - sinT2);
    }
    float x = 1.0f - cosX;
    return r0 + (1.0f - r0) * x * x * x * x * x;
}

/* One soft-shadow sample (raytracing.cl:99-110): angles from the two xorshift values -- fp64 products rounded to
 * fp32, M_PI being a double constant -- a point on the light sphere, and the unit direction / distance to it. */
__device__ __forceinline__ f3 wt_light_sample_dir(float4 l0, float4 l1, float u1, float u2, f3 from, float& dist) {
    float sp_, cp_, st_, ct_;
    wt_sincos_angle<false>(u2, sp_, cp_);    /* phi   = pi * u2   */
    wt_sincos_angle<true>(u1, st_, ct_);     /* theta = 2 pi * u1 */
#if WT_STRICT
    float sx = l1.w * sp_ * ct_;
    float sy = l1.w * sp_ * st_;
    float sz = l1.w * cp_;
    const f3 to = mk3(l0.x, l0.y, l0.z) + mk3(sx, sy, sz);
    return wt_normalize_len(to - from, dist);
#else   /* (centre - from) + offset instead of (centre + offset) - from: the first term is shared by the samples of a light, the
         * offsets fuse into three FMAs -- 5 instructions less per sample, the sample point moves by an ulp of the distance */
    const f3 lf = mk3(l0.x - from.x, l0.y - from.y, l0.z - from.z);
    const float rs = l1.w * sp_;
    return wt_normalize_len(mk3(__builtin_fmaf(rs, ct_, lf.x), __builtin_fmaf(rs, st_, lf.y), __builtin_fmaf(l1.w, cp_, lf.z)), dist);
#endif
}

/* ---- one light at a shaded hit (raytracing.cl:87-136), shared by the three forms of the shadow phase ----------
 * wt_light_terms: distance and direction to the light CENTRE, the Blinn-Phong factors (they ignore the material colour,
 * raytracing.cl:129-135) and `need`: false when the light's term is exactly +0 whatever its shadow rays say -- a
 * surface whose specular and diffuse coefficients are both zero (glass), every other factor being finite (a
 * non-finite one keeps the slow path, so 0 * NaN still poisons the pixel as in the reference).
 * wt_light_add: the term itself, `soft` = sum of the light's WT_SOFT shadow factors. */
struct light_terms { float dl, spec, diff; bool need; };
__device__ __forceinline__ light_terms wt_light_terms(float4 l0, f3 ip, f3 nrm, f3 view, float shininess, float ks, float kd) {
    light_terms L;
#if WT_STRICT
    const f3 sdir = wt_normalize_len(mk3(l0.x, l0.y, l0.z) - ip, L.dl);
    const f3 hv = wt_normalize(view + sdir);
    const float sdot = dot3(nrm, hv);
    const float ddot = dot3(nrm, sdir);
#else   /* neither unit vector is needed by itself: n.h = n.(view + v rs) rsq(|view + v rs|^2), n.l = (n.v) rs -- five instructions less */
    const f3 lv = mk3(l0.x, l0.y, l0.z) - ip;
    const float d2 = dot3(lv, lv);
    const float rs = __builtin_amdgcn_rsqf(d2);
    L.dl = d2 * rs;
    const f3 hu = wt_madd3(lv, rs, view);
    const float sdot = dot3(nrm, hu) * __builtin_amdgcn_rsqf(dot3(hu, hu));
    const float ddot = dot3(nrm, lv) * rs;
#endif
    L.spec = wt_pow(0.0f > sdot ? 0.0f : sdot, shininess);        /* max(0, x) as `a > b ? a : b` */
    L.diff = 0.0f > ddot ? 0.0f : ddot;
    /* The light's term is ((lrgb ks) spec) + ((lrgb kd) diff) (raytracing.cl:129-135): with ks or spec zero AND kd or diff zero it is
     * exactly 0 whatever the shadow factor -- glass (ks = kd = 0), but also a mirror away from its highlight (kd = 0 and
     * pow(n.h, 100) underflows to 0 below n.h = 0.36: most of render.map's mirror wall) or a light behind a matte surface.  Only a
     * wave that holds such a lane evaluates the finiteness side of the rule. */
    L.need = true;
    const bool zero = (ks == 0.0f || L.spec == 0.0f) && (kd == 0.0f || L.diff == 0.0f);
    if (__builtin_amdgcn_ballot_w64(zero) != 0)
        L.need = !(zero && L.dl * L.dl > 0.0f && L.dl * L.dl < INFINITY && fabsf(L.spec) < INFINITY && fabsf(L.diff) < INFINITY &&
                   fabsf(ks) < INFINITY && fabsf(kd) < INFINITY);      /* (`< INFINITY` is false for NaN too) */
#if !WT_STRICT  /* everything of the light's term but its shadow factor is known here: ONE weight (ks spec + kd diff) / (2 d^2) travels across
                 * the shadow phase in `spec` instead of spec and diff (three registers less, and wt_light_add is a multiply and three FMAs) */
    L.spec = ((rs * rs) * (1.0f / (float)WT_SOFT)) * __builtin_fmaf(ks, L.spec, kd * L.diff);
    L.diff = 0.0f;
#endif
    return L;
}
__device__ __forceinline__ f3 wt_light_add(f3 rgb, float4 l1, float soft, float dl, float spec, float diff, float ks, float kd) {
#if !WT_STRICT  /* the two terms share everything but ks spec and kd diff: one weight, three FMAs (21 -> 4 instructions per light here);
                 * a zero-coefficient surface still receives exactly rgb + 0 (see wt_light_terms) */
    return wt_madd3(mk3(l1.x, l1.y, l1.z), spec * soft, rgb);      /* `spec` carries the light's whole weight, see wt_light_terms */
#endif
    const float ssr = soft / (float)WT_SOFT;
    const float d2 = dl * dl;
    f3 lrgb = mk3(wt_div(l1.x, d2), wt_div(l1.y, d2), wt_div(l1.z, d2));
    lrgb = lrgb * ssr;
    rgb = wt_madd3(lrgb * ks, spec, rgb);
    return wt_madd3(lrgb * kd, diff, rgb);
}

/* wave-uniform geometry fetch: LDS broadcast read or (large scenes) global/L2 */
template <bool GEOM_LDS>
__device__ __forceinline__ float4 wt_geom(const whitted_params& P, const float4* sg, unsigned i) {
    if (GEOM_LDS) return sg[i];
    return ((const float4*)P.geom)[i];
}
/* ---- moving spheres (whitted_params.h: ss_disp, ss_times): EVERY read of a sphere's float4 goes through wt_sphere_at, which returns the sphere as
 * the lane's sub-sample sees it -- centre fmaf(t, d_i, c_i) per component, one rounding in both builds (the host's clw_host_spheres_at does the
 * same), radius and the transparency bit untouched.  `on` is a compile-time constant: true in the WT_F_MOVE flavours only, false in every other kernel,
 * whose code is then the plain fetch it was; the displacement is an LDS broadcast read behind the staged geometry (or a uniform global load).
 * A moving sphere's centre is a per-lane value: every ballot around a sphere test is an early-out over per-lane predicates (no lane's result
 * depends on what another lane's test gave), and the one wave-level decision that reads centres, wt_sphere_candidates, is skipped. */
struct wt_motion { bool on; float t; unsigned off; };   /* off: float4 index of the staged table in the LDS stream (= geom_f4) */
template <bool GEOM_LDS>
__device__ __forceinline__ float4 wt_sphere_at(const whitted_params& P, const float4* sg, unsigned i, const wt_motion& mv) {
    float4 s = wt_geom<GEOM_LDS>(P, sg, i);
    if (mv.on) {
        const float4 dd = GEOM_LDS ? sg[mv.off + i] : ((const float4*)P.ss_disp)[i];
        s.x = __builtin_fmaf(mv.t, dd.x, s.x); s.y = __builtin_fmaf(mv.t, dd.y, s.y); s.z = __builtin_fmaf(mv.t, dd.z, s.z);
    }
    return s;
}


/* (the WT_F_* flags of FLAGS and WT_SHAPE_FLAGS: whitted_params.h) */
/* the flavours that take the seed offset and the accumulation branch only as their WT_F_ACC twin (tools/kernel_stats.py against the parent:
 * profiles/r10_ab_experiments.txt) */
constexpr bool wt_acc_flagged(int flags) { return WT_STRICT != 0 && (flags & WT_F_DEEP) == 0 && (flags & (WT_F_COUNT | WT_F_GRID)) != 0; }

/* ---- the scene's primitive counts: launch parameters, or compile-time constants (FLAGS & WT_F_SHAPE) ----------------------------
 * A small scene's loops over 4 spheres, 2 planes and 3 lights are mostly loop control, guards and selects around little arithmetic.
 * The shaped flavour carries ns, np and nl in FLAGS bits 9-11, 12-13 and 14-16: every sphere, plane and light loop of the hot path
 * unrolls, the geometry offsets and the early-out ballots' positions become constants, and the side-table branch folds (the shim
 * launches it only when the light / plane side table is on or there are no planes).  Same operations in the same order: the frame is
 * the generic kernel's, bit for bit.  (WT_SHAPE_FLAGS of whitted_params.h: launch_plan.c picks the kernel from the prepared scene.) */
template <int FLAGS>
struct wt_shape {
    static constexpr bool on = (FLAGS & WT_F_SHAPE) != 0;
    static constexpr unsigned cns = ((unsigned)FLAGS >> 9) & 7u, cnp = ((unsigned)FLAGS >> 12) & 3u, cnl = ((unsigned)FLAGS >> 14) & 7u;
    static __device__ __forceinline__ unsigned ns(const whitted_params& P) { return on ? cns : P.ns; }
    static __device__ __forceinline__ unsigned np(const whitted_params& P) { return on ? cnp : P.np; }
    static __device__ __forceinline__ unsigned nl(const whitted_params& P) { return on ? cnl : P.nl; }
    static __device__ __forceinline__ bool lpt(const whitted_params& P) { return on ? true : P.lpt != 0u; }
};


/* ---- uniform-grid traversal over the spheres (big scenes; FLAGS & WT_F_GRID) ------------------------------
 * 3-D DDA through the cells the ray crosses; every sphere registered in a cell is tested with the SAME
 * wt_sphere arithmetic as the brute-force loop, so the t values are bit-identical and only the number of
 * tests changes.  Nearest hit: ties keep the lower sphere index, like the reference's in-order scan with
 * its strict `_t >= t` (primitives.cl:342).  Shadow rays: a transparent sphere spanning several cells is
 * counted once -- in the first cell of its cell box that the walk enters. */
/* finite origin and direction, direction not all zero: what the DDA needs to have cells to walk */
__device__ __forceinline__ bool wt_ray_walkable(f3 o, f3 d) {
    const float chk = (o.x - o.x) + (o.y - o.y) + (o.z - o.z) + (d.x - d.x) + (d.y - d.y) + (d.z - d.z);   /* NaN iff any is NaN / inf, else 0 */
    return chk == 0.0f && (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f);
}
/* DIAGNOSTIC (-DWT_GRIDSTATS=1 with counters enabled; never the product): lane- and wave-level step counts of the grid
 * walks in counter words 10..17 -- nearest {walks, lane cell steps, wave cell steps, sphere tests}, shadow the same. */
#ifndef WT_GRIDSTATS
#define WT_GRIDSTATS 0
#endif
#if WT_GRIDSTATS
#define WT_GSTAT(idx_lane, idx_wave) do { if (P.counters) { const unsigned long long m_ = __builtin_amdgcn_ballot_w64(true); \
        if (__lane_id() == (unsigned)__builtin_ctzll(m_)) { if ((idx_lane) >= 0) atomicAdd(P.counters + (idx_lane), (unsigned long long)__builtin_popcountll(m_)); \
                                                            if ((idx_wave) >= 0) atomicAdd(P.counters + (idx_wave), 1ull); } } } while (0)
#else
#define WT_GSTAT(idx_lane, idx_wave) do { } while (0)
#endif
struct grid_walk {
    int c[3], st[3];
    float tn[3], td[3];
    float texit;
};
__device__ __forceinline__ bool wt_grid_begin(const whitted_params& P, f3 o, f3 d, float tend, grid_walk& w) {
    /* ONE reciprocal per axis (v_rcp_f32 in the fast build): the walk's boundary parameters only decide WHICH cells are visited, and a
     * sphere is listed in every cell its padded box touches (scene_prep.c sphere_cells: 1e-3 cell), so an ulp in tn / td is harmless.
     * (The nine IEEE divides this replaces were 90 of the ~390 instructions a shadow ray costs at C4.) */
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    float inv[3];
    float t0 = 0.0f, t1 = tend;
#pragma unroll
    for (int a = 0; a < 3; a++) {
#if WT_STRICT
        inv[a] = 1.0f / dd[a];
#else
        inv[a] = __builtin_amdgcn_rcpf(dd[a]);
#endif
        const float lo = P.grid_min[a], hi = P.grid_min[a] + P.grid_cell[a] * (float)P.grid_res[a];
        const float ta = (lo - oo[a]) * inv[a], tb = (hi - oo[a]) * inv[a];
        t0 = fmaxf(t0, fminf(ta, tb));           /* fminf/fmaxf drop the NaN of 0 * inf (ray parallel to a slab it starts on) */
        t1 = fminf(t1, fmaxf(ta, tb));
        if (dd[a] == 0.0f && (oo[a] < lo || oo[a] > hi)) return false;
    }
    if (!(t0 <= t1)) return false;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float p = oo[a] + dd[a] * t0;
        int c = (int)floorf((p - P.grid_min[a]) * P.grid_inv[a]);
        c = min(max(c, 0), P.grid_res[a] - 1);
        w.c[a] = c;
        if (dd[a] != 0.0f) {
            const bool up = dd[a] > 0.0f;
            w.st[a] = up ? 1 : -1;
            w.tn[a] = (P.grid_min[a] + P.grid_cell[a] * (float)(up ? c + 1 : c) - oo[a]) * inv[a];
            w.td[a] = P.grid_cell[a] * fabsf(inv[a]);
        } else {
            w.st[a] = 0; w.tn[a] = INFINITY; w.td[a] = INFINITY;
        }
    }
    return true;
}
/* cell index of the current cell; sets texit = parameter at which the ray leaves it */
__device__ __forceinline__ unsigned wt_grid_cell(const whitted_params& P, grid_walk& w) {
    w.texit = fminf(w.tn[0], fminf(w.tn[1], w.tn[2]));
    return ((unsigned)w.c[2] * (unsigned)P.grid_res[1] + (unsigned)w.c[1]) * (unsigned)P.grid_res[0] + (unsigned)w.c[0];
}
/* step to the next cell; false when the walk leaves the grid */
__device__ __forceinline__ bool wt_grid_next(const whitted_params& P, grid_walk& w) {
    /* the axis whose boundary comes first (ties: x before y before z), as selects -- the walk is divergent enough
     * without a three-way branch per cell */
    const bool a0 = w.tn[0] <= w.tn[1] && w.tn[0] <= w.tn[2];
    const bool a1 = !a0 && w.tn[1] <= w.tn[2];
    const bool a2 = !a0 && !a1;
    /* The walk is finite by construction: every step moves ONE axis by its fixed +-1, so after at most
     * res[0] + res[1] + res[2] steps a cell index leaves [0, res).  A step that would not move (the selected axis
     * has st == 0: its boundary parameter is INF or the comparisons met a NaN) means no further cell is reachable
     * in float range, and the walk ends there. */
    const int moved = a0 ? w.st[0] : (a1 ? w.st[1] : w.st[2]);
    w.c[0] += a0 ? w.st[0] : 0;  w.c[1] += a1 ? w.st[1] : 0;  w.c[2] += a2 ? w.st[2] : 0;
    w.tn[0] = a0 ? w.tn[0] + w.td[0] : w.tn[0];
    w.tn[1] = a1 ? w.tn[1] + w.td[1] : w.tn[1];
    w.tn[2] = a2 ? w.tn[2] + w.td[2] : w.tn[2];
    return moved != 0 && (unsigned)w.c[0] < (unsigned)P.grid_res[0] && (unsigned)w.c[1] < (unsigned)P.grid_res[1] &&
           (unsigned)w.c[2] < (unsigned)P.grid_res[2];
}

/* The walk is a chain of dependent loads -- cell header, then the entries -- at ~0.3 us of L2 latency each, and
 * that latency, not arithmetic, is what a big scene costs.  So (1) every cell-list entry carries its sphere
 * (grid_geom[k] = geom[grid_items[k]]): one load per test, the index is fetched only for a hit; (2) the header of
 * the NEXT cell is requested before the entries of the current one are tested. */
/* (Measured and dropped, round 2: a 64-byte record per cell with its first two spheres inline -- one level of dependent
 * loads instead of two -- is SLOWER, 2.6-3.7 ms against 2.3 ms at C4: most cells of a walk are empty, and an empty cell
 * then costs 48 bytes per lane instead of the 8-byte header; and walking the two samples of a light together
 * loses more to its registers than it gains from the overlap.) */
struct grid_cellrange { unsigned b, e; };
__device__ __forceinline__ grid_cellrange wt_grid_range(const whitted_params& P, unsigned c) {
    grid_cellrange r; r.b = P.grid_start[c]; r.e = P.grid_start[c + 1]; return r;
}

/* nearest sphere along the ray: returns its index or -1; tbest = its t */
__device__ __forceinline__ int wt_grid_nearest(const whitted_params& P, const rayq& r, float& tbest) {
    grid_walk w;
    tbest = INFINITY;
    int best = -1;
    if (!wt_ray_walkable(r.o, r.d)) {
        /* a NaN / infinite / zero ray (a pixel already poisoned by normalize(0) and the like) has no cells to walk:
         * it takes the reference's in-order scan, whose comparisons define what such a ray "hits" (every test passes
         * with t = NaN and the last primitive wins), so the pixel ends exactly as in the linear-scan build */
        for (unsigned i = 0; i < P.ns; i++) {
            const float4 s = ((const float4*)P.geom)[i];
            float t;
            if (wt_sphere_dir(wt_sphere_pre(r.o, s), r.d, r.a4, r.a2, t) && !(t >= tbest)) { tbest = t; best = (int)i; }
        }
        return best;
    }
    if (!wt_grid_begin(P, r.o, r.d, INFINITY, w)) return -1;
    grid_cellrange cur = wt_grid_range(P, wt_grid_cell(P, w));
    WT_GSTAT(10, -1);
    for (;;) {
        WT_GSTAT(11, 12);
        const float texit = w.texit;
        grid_walk nw = w;
        const bool more = wt_grid_next(P, nw);
        grid_cellrange nxt; nxt.b = 0u; nxt.e = 0u;
        if (more) nxt = wt_grid_range(P, wt_grid_cell(P, nw));       /* in flight while this cell is tested */
        for (unsigned k = cur.b; k < cur.e; k++) {
            WT_GSTAT(13, -1);
            const float4 s = ((const float4*)P.grid_geom)[k];
            const sph_pre pre = wt_sphere_pre(r.o, s);
            float t;
            if (wt_sphere_dir(pre, r.d, r.a4, r.a2, t)) {
                /* first-in-index-order wins on equal t; a NaN t is accepted like the reference's `!(t >= tbest)` */
                if (!(t > tbest)) {
                    const int i = (int)P.grid_items[k];
                    if (!(t >= tbest) || i < best) { tbest = t; best = i; }
                }
            }
        }
        if (best >= 0 && tbest <= texit) break;        /* the hit lies inside the cells already walked */
        if (!more) break;
        w = nw; cur = nxt;
    }
    return best;
}

/* Is an OPAQUE sphere hit at t <= tl?  (findLightIntersection's visibility check of a light sphere the ray meets at tl,
 * primitives.cl:296-318, over the grid instead of all ns spheres: a 10 000-sphere scan per ray made the few tiles that SEE
 * a light sphere the longest-living waves of a C4 frame -- 2 ms, the whole kernel.)  Same test per sphere as the scan; a
 * sphere met at t <= tl is listed in the cell the ray is in at t, and that cell is entered at a parameter <= tl. */
__device__ __forceinline__ bool wt_grid_occluded(const whitted_params& P, const rayq& r, float tl) {
    if (!wt_ray_walkable(r.o, r.d)) {           /* see wt_grid_nearest: the in-order scan */
        bool blocked = false;
        for (unsigned i = 0; i < P.ns; i++) {
            const float4 s = ((const float4*)P.geom)[i];
            float t;
            if (wt_sphere_dir(wt_sphere_pre(r.o, s), r.d, r.a4, r.a2, t) && t <= tl && !(__float_as_uint(s.w) >> 31)) blocked = true;
        }
        return blocked;
    }
    grid_walk w;
    if (!wt_grid_begin(P, r.o, r.d, INFINITY, w)) return false;
    grid_cellrange cur = wt_grid_range(P, wt_grid_cell(P, w));
    for (;;) {
        const float texit = w.texit;
        grid_walk nw = w;
        const bool more = wt_grid_next(P, nw) && !(texit > tl);
        grid_cellrange nxt; nxt.b = 0u; nxt.e = 0u;
        if (more) nxt = wt_grid_range(P, wt_grid_cell(P, nw));
        for (unsigned k = cur.b; k < cur.e; k++) {
            const float4 s = ((const float4*)P.grid_geom)[k];
            float t;
            if (wt_sphere_dir(wt_sphere_pre(r.o, s), r.d, r.a4, r.a2, t) && t <= tl && !(__float_as_uint(s.w) >> 31)) return true;
        }
        if (!more) return false;
        w = nw; cur = nxt;
    }
}

/* The shadow walk as a state machine -- begin, then one cell per step -- so that a lane can interleave walks of rays it
 * fetches from a wave-wide pool (the grid builds' shading phase) as well as run one to the end (wt_grid_shadow). */
struct grid_shadow_state { grid_walk w; grid_cellrange cur; int pc0, pc1, pc2; };
__device__ __forceinline__ bool wt_gs_begin(const whitted_params& P, f3 o, f3 d, float tl, grid_shadow_state& st) {
#ifdef WT_HACK_NOSHADOWWALK      /* DIAGNOSTIC only (wrong images): what does everything but the shadow walks cost? */
    return false;
#endif
    if (!wt_grid_begin(P, o, d, tl, st.w)) return false;
    st.pc0 = st.pc1 = st.pc2 = -1;                     /* previous cell of the walk */
    st.cur = wt_grid_range(P, wt_grid_cell(P, st.w));
    WT_GSTAT(14, -1);
    return true;
}
/* tests the current cell and moves to the next one; true when the walk is over (op then holds the ray's factor) */
__device__ __forceinline__ bool wt_gs_step(const whitted_params& P, f3 o, f3 d, float a4, float a2, float tl,
                                           grid_shadow_state& st, float& op) {
    WT_GSTAT(15, 16);
    const float texit = st.w.texit;
    grid_walk nw = st.w;
    const bool more = wt_grid_next(P, nw) && texit < tl;   /* the rest of the walk lies beyond the light sample */
    grid_cellrange nxt; nxt.b = 0u; nxt.e = 0u;
    if (more) nxt = wt_grid_range(P, wt_grid_cell(P, nw));
#ifdef WT_HACK_NOSHADOWTESTS     /* DIAGNOSTIC only (wrong images): the traversal without its sphere tests */
    st.cur.e = st.cur.b;
#endif
    /* one entry of the cell; true when it blocks the ray */
    auto entry = [&](const float4 s, const unsigned k) -> bool {
        const sph_pre pre = wt_sphere_pre(o, s);      /* the FULL quadratic: see wt_grid_shadow */
        float t;
        if (wt_sphere_dir(pre, d, a4, a2, t) && !(t >= tl)) {
            if (!(__float_as_uint(s.w) >> 31)) return true;                          /* opaque: blocked */
            const unsigned i = P.grid_items[k];
            const unsigned lo = P.grid_box[2 * i], hi = P.grid_box[2 * i + 1];
            const bool seen = st.pc0 >= (int)(lo & 1023u) && st.pc0 <= (int)(hi & 1023u) &&
                              st.pc1 >= (int)((lo >> 10) & 1023u) && st.pc1 <= (int)((hi >> 10) & 1023u) &&
                              st.pc2 >= (int)(lo >> 20) && st.pc2 <= (int)(hi >> 20);
            if (!seen) op *= P.through;                             /* counted once per sphere */
        }
        return false;
    };
    /* the entries two at a time: both loads are in flight before the first test (a cell of C4 holds 1.7 spheres on average, and the
     * walk waits for every load it issues) */
    for (unsigned k = st.cur.b; k < st.cur.e; k += 2u) {
        WT_GSTAT(17, 21);
        const bool two = k + 1u < st.cur.e;
        const float4 s0 = ((const float4*)P.grid_geom)[k];
        const float4 s1 = ((const float4*)P.grid_geom)[two ? k + 1u : k];
        if (entry(s0, k)) { op = 0.0f; return true; }
        if (two && entry(s1, k + 1u)) { op = 0.0f; return true; }
    }
    if (!more) return true;
    st.pc0 = st.w.c[0]; st.pc1 = st.w.c[1]; st.pc2 = st.w.c[2];
    st.w = nw; st.cur = nxt;
    return false;
}

/* testShadowPath over the spheres (primitives.cl:404-420): 0 when an opaque sphere lies before `tl`,
 * else 0.8^(number of transparent spheres before tl).
 * Shadow rays that walk the grid keep the FULL quadratic in both builds (a4 / a2 from wt_rayq<false>, not the fast build's a = 1 of
 * wt_shadow_*): grid scenes are big scenes, where rays start up to a hundred units from the spheres they pass and b*b and 4ac agree to
 * 5-7 digits -- 3e-7 of a is not below that noise (the same rule the other rays of a big scene follow, see wt_rayq). */
__device__ __forceinline__ float wt_grid_shadow(const whitted_params& P, f3 o, f3 d, float a4, float a2, float tl) {
    float op = 1.0f;
    if (!wt_ray_walkable(o, d)) {           /* see wt_grid_nearest: the in-order scan of testShadowPath */
        for (unsigned i = 0; i < P.ns; i++) {
            const float4 s = ((const float4*)P.geom)[i];
            float t;
            if (wt_sphere_dir(wt_sphere_pre(o, s), d, a4, a2, t) && !(t >= tl)) {
                if (!(__float_as_uint(s.w) >> 31)) return 0.0f;
                op *= P.through;
            }
        }
        return op;
    }
    grid_shadow_state st;
    if (!wt_gs_begin(P, o, d, tl, st)) return op;
    while (!wt_gs_step(P, o, d, a4, a2, tl, st, op)) { }
    return op;
}


/* The WT_SOFT = 2 samples of ONE light as ONE walk (scenes whose grid lists every sphere a light radius beyond its box, P.grid_pair).
 * Both rays leave `o` and end ON the light sphere (centre at distance lc along the unit direction dc, radius <= the grid's reg_pad):
 * the point of ray q at fraction s of its length is o + s (L - o) + s offset_q, within s r of the point o + s (L - o) of the ray to
 * the light's centre.  So a sphere that ray q meets before its sample contains a point within r of the CENTRE ray's segment [0, lc],
 * its widened box contains that segment point, and the cell the centre ray is in there lists it: walking the centre ray's cells and
 * testing both rays against every entry finds every hit the two per-ray walks of wt_grid_shadow find -- and a hit is a hit whichever
 * cell offered the sphere (same wt_sphere_dir per test: same t, same `t < tl`).  A transparent sphere is counted once per ray, in the
 * first cell of its cell box the walk enters (the cells of a box a straight walk visits are consecutive); the factors are all
 * P.through, so their order does not matter.  Half the walks, the origin-only half of every test shared by the two rays.
 * op[q] enters 1 (ray to trace) or 0 and leaves as the ray's factor.  (Measured and dropped: this function as the ONLY walk, called once per
 * sample where the lights are too big for sharing -- the pair 5 % slower through the pass loop around it.) */
__device__ __forceinline__ void wt_grid_shadow_pair(const whitted_params& P, f3 o, f3 dc, float lc, const f3 (&d)[2], const float (&a4)[2],
                                                    const float (&a2)[2], const float (&tl)[2], float (&op)[2]) {
    if (!wt_ray_walkable(o, dc) || !wt_ray_walkable(o, d[0]) || !wt_ray_walkable(o, d[1]) || !(lc - lc == 0.0f)) {
        /* (a NaN / infinite / zero ray has no cells to walk: the reference's in-order scan, see wt_grid_nearest) */
        for (unsigned i = 0; i < P.ns; i++) {
            const float4 s = ((const float4*)P.geom)[i];
            const sph_pre pre = wt_sphere_pre(o, s);
#pragma unroll
            for (int q = 0; q < 2; q++) {
                float t;
                if (op[q] != 0.0f && wt_sphere_dir(pre, d[q], a4[q], a2[q], t) && !(t >= tl[q])) op[q] = (__float_as_uint(s.w) >> 31) ? op[q] * P.through : 0.0f;
            }
        }
        return;
    }
    grid_shadow_state st;
    if (!wt_gs_begin(P, o, dc, lc, st)) return;
    for (;;) {
        const float texit = st.w.texit;
        grid_walk nw = st.w;
        const bool more = wt_grid_next(P, nw) && texit < lc;
        grid_cellrange nxt; nxt.b = 0u; nxt.e = 0u;
        if (more) nxt = wt_grid_range(P, wt_grid_cell(P, nw));
        auto entry = [&](const float4 s, const unsigned k) {
            const sph_pre pre = wt_sphere_pre(o, s);          /* shared by the two rays */
            bool hit[2];
#pragma unroll
            for (int q = 0; q < 2; q++) { float t; hit[q] = op[q] != 0.0f && wt_sphere_dir(pre, d[q], a4[q], a2[q], t) && !(t >= tl[q]); }
            if (hit[0] || hit[1]) {
                if (!(__float_as_uint(s.w) >> 31)) { if (hit[0]) op[0] = 0.0f; if (hit[1]) op[1] = 0.0f; }    /* opaque: blocked */
                else {
                    const unsigned i = P.grid_items[k];
                    const unsigned lo = P.grid_box[2 * i], hi = P.grid_box[2 * i + 1];
                    const bool seen = st.pc0 >= (int)(lo & 1023u) && st.pc0 <= (int)(hi & 1023u) &&
                                      st.pc1 >= (int)((lo >> 10) & 1023u) && st.pc1 <= (int)((hi >> 10) & 1023u) &&
                                      st.pc2 >= (int)(lo >> 20) && st.pc2 <= (int)(hi >> 20);
                    if (!seen) { if (hit[0]) op[0] *= P.through; if (hit[1]) op[1] *= P.through; }
                }
            }
        };
        for (unsigned k = st.cur.b; k < st.cur.e; k += 2u) {
            const bool two = k + 1u < st.cur.e;
            const float4 s0 = ((const float4*)P.grid_geom)[k];
            const float4 s1 = ((const float4*)P.grid_geom)[two ? k + 1u : k];
            entry(s0, k);
            if (two) entry(s1, k + 1u);
        }
        if ((op[0] == 0.0f && op[1] == 0.0f) || !more) return;
        st.pc0 = st.w.c[0]; st.pc1 = st.w.c[1]; st.pc2 = st.w.c[2];
        st.w = nw; st.cur = nxt;
    }
}


/* ---- light visibility classes: which shadow samples need a ray at all ------------------------------------------------------
 * The WT_SOFT samples of a light (raytracing.cl:96-110) lie ON the light sphere (centre L, radius rho), so every shadow ray of
 * the light stays inside the cone K with apex ip through that sphere (half-angle alpha, sin alpha = rho / |L - ip|) and ends inside
 * the ball B(L, rho).  For one sphere (c, R) of the scene, with w = c - ip, s / p its axial / radial coordinates about the
 * cone's axis and q = p cos(alpha) - s sin(alpha) (a lower bound of its centre's distance from K):
 *   CLEAR   no ray of the cone can report a hit in front of its sample: q > R (the sphere lies beside the cone), or the
 *           nearest point of K is the apex itself and |w| > R (the sphere lies behind the shading point -- its OWN sphere, an
 *           epsilon away), or |w| - R > |L - ip| + rho (the sphere lies beyond the light);
 *   FULL    EVERY ray of the cone reports a hit in front of its sample: the disc the cone cuts out at the sphere centre's axial
 *           position lies inside the sphere, the origin outside it and the sphere wholly in front of B;
 *   else the sphere is PARTIAL and the light's samples must be traced.
 * A light without partial spheres and without a plane that can block it (the light / plane side table) has the SAME shadow
 * factor for every sample, whatever the random numbers: 0 if an opaque sphere is FULL, else 0.8^(number of transparent FULL
 * spheres) multiplied up in index order like testShadowPath does (primitives.cl:404-420) -- the factor the traced rays would
 * return, bit for bit, without their sin / cos, normalisation and intersection tests.  The random numbers are still drawn.
 * Every comparison carries a margin that covers (a) the rounding of the reference's own evaluation of b*b - 4ac and t for rays
 * of the cone (< 7.5e-7 |w|^2 in D/4, derivation in DESIGN.md section 4), (b) the rounding of the quantities below and (c) the
 * rounding of the sample point itself (rho is inflated by 1e-4 rho + 2e-7 |L|_1); 1e-5 |w|^2 is used for (a) + (b).  A comparison
 * that meets a NaN or an infinity is false, which makes the sphere PARTIAL: when in doubt the rays are traced.
 * tests/test_gpu_parity.py runs the counting build with P.vis == 2, which classifies AND traces and counts the lights whose
 * traced factors differ from the class's (must be zero). */
template <bool GEOM_LDS, int LCH>
__device__ __forceinline__ void wt_light_vis(const whitted_params& P, const float4* sg, unsigned g_pln, unsigned g_lgt, unsigned lb,
                                             f3 ip, const bool (&want)[LCH], unsigned chunk, bool (&known)[LCH], float (&opu)[LCH],
                                             const wt_motion mv = wt_motion{false, 0.0f, 0u}) {
    f3 lv[LCH];
    float rs[LCH], dl[LCH], rho[LCH], sa[LCH], ca2[LCH];
    bool live[LCH], unk[LCH], blk[LCH], pok[LCH];
#pragma unroll
    for (int k = 0; k < LCH; k++) {
        float4 l0 = make_float4(0, 0, 0, 0);
        float lrad = 0.0f;
        if (lb + k < P.nl) {                                     /* wave-uniform; `want` is false for a light that does not exist */
            l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (lb + k));
            lrad = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (lb + k) + 1).w;
        }
        lv[k] = mk3(l0.x, l0.y, l0.z) - ip;
        const float d2 = dot3(lv[k], lv[k]);
        rs[k] = __builtin_amdgcn_rsqf(d2);
        dl[k] = d2 * rs[k];
        rho[k] = __builtin_fmaf(fabsf(lrad), 1.0001f, __builtin_fmaf(2e-7f, fabsf(l0.x) + fabsf(l0.y) + fabsf(l0.z), 1e-30f));
        sa[k] = rho[k] * rs[k];
        ca2[k] = __builtin_fmaf(-sa[k], sa[k], 1.0f);
        live[k] = want[k] && sa[k] < 0.5f;              /* (false for a NaN too) */
        unk[k] = want[k] && !live[k];
        blk[k] = false; pok[k] = true; opu[k] = 1.0f;
    }
    /* planes: none may be able to block a sample (same predicate as wt_shadow_batch's wave-level skip) */
    if (P.np != 0u) {
        if (!P.lpt || chunk == ~0u || LCH != 3) {
#pragma unroll
            for (int k = 0; k < LCH; k++) pok[k] = false;
        } else {
            for (unsigned i = 0; i < P.np; i++) {
                const float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
                const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
                const float4 mu = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * P.np + 2 * P.nl + chunk * P.np + i);
                const float num = wt_plane_pre(ip, n, p0);
                const float mus[3] = {mu.x, mu.y, mu.z};
                const float an = 1e-5f * fabsf(num) * mu.w;
#pragma unroll
                for (int k = 0; k < LCH && k < 3; k++)
                    pok[k] = pok[k] && (num * mus[k] < 0.0f) && (fabsf(mus[k]) > __builtin_fmaf(4e-6f, dl[k], an));
            }
        }
    }
    for (unsigned i = 0; i < P.ns; i++) {
        const float4 s4 = wt_sphere_at<GEOM_LDS>(P, sg, i, mv);
        const f3 w = mk3(s4.x, s4.y, s4.z) - ip;                 /* = -(from - centre) of primitives.cl:173, exactly */
        const float ww = dot3(w, w), R2 = fabsf(s4.w);
        const float slack = __builtin_fmaf(1e-5f, ww, 1e-30f);
        const float cc = ww - R2;
        const float iR = __builtin_amdgcn_rsqf(R2), Rr = R2 * iR;   /* R = 0: NaN, the sphere ends up PARTIAL */
        const float Rm = __builtin_fmaf(slack, iR, Rr) * 1.00001f;  /* (R + slack / R)^2 >= R^2 + 2 slack */
        float sk[LCH], p2k[LCH];
        bool open[LCH], any = false;
#pragma unroll
        for (int k = 0; k < LCH; k++) {
            sk[k] = dot3(w, lv[k]) * rs[k];
            p2k[k] = __builtin_fmaf(-sk[k], sk[k], ww);
            const float t1 = __builtin_fmaf(sk[k], sa[k], Rm);
            const bool clear = (t1 < 0.0f) || (p2k[k] * ca2[k] > t1 * t1 * 1.00001f);      /* q > R, with margin */
            open[k] = live[k] && !clear;
            any |= open[k];
        }
        if (__builtin_amdgcn_ballot_w64(any) == 0) continue;           /* the sphere is beside every cone of the wave */
#pragma unroll
        for (int k = 0; k < LCH; k++) {
            if (open[k]) {
                const float s = sk[k], p2 = p2k[k];
                /* behind the apex: s cos(alpha) + p sin(alpha) <= 0 (region shrunk by 1e-3), and the origin outside the sphere */
                const bool apex = s < 0.0f && (p2 * sa[k] * sa[k] <= s * s * ca2[k] * 0.999f) && cc > slack;
                const float far_ = __builtin_fmaf(dl[k] + rho[k], 1.00002f, Rm);
                const bool beyond = ww > far_ * far_ * 1.00001f;
                if (!(apex || beyond)) {
                    const float ica = __builtin_amdgcn_rsqf(ca2[k]);                          /* 1 / cos(alpha) */
                    const float p = __builtin_amdgcn_sqrtf(__builtin_fmaf(2e-6f, ww, fmaxf(p2, 0.0f)));
                    const float e = __builtin_fmaf(s * 1.0001f, sa[k] * ica, p);             /* p + s tan(alpha) */
                    const bool full = s > 0.0f && cc > slack && (e * e < __builtin_fmaf(-2.0f, slack, R2)) &&
                                      (s * ica * 1.0001f < dl[k] - rho[k]);
                    if (!full) unk[k] = true;
                    else if (__float_as_uint(s4.w) >> 31) opu[k] *= P.through;
                    else blk[k] = true;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < LCH; k++) {
        known[k] = want[k] && (blk[k] || (!unk[k] && pok[k]));
        if (blk[k]) opu[k] = 0.0f;
    }
}

/* ---- which spheres can the shadow rays of a WAVE meet at all?  (scenes of 16..64 spheres, deep builds: C3's 64 glass spheres) --------------
 * The batch tests every sphere against six rays per lane although the rays of a wave -- from shading points close together, to lights of
 * radius 0.1 -- pass near a handful of them.  Every ray of the batch runs from one of the wave's shading points (all inside the ball
 * B(m, rho): m = centre of their bounding box, rho = its half diagonal) to a point on a light sphere B(L, r), so it lies in the convex hull of the two
 * balls, which lies within max(rho, r) of the segment m -> L.  A sphere (c, R) farther than R + max(rho, r) from that segment (plus a margin a
 * thousand times the rounding involved) cannot be met by any of them in front of its sample: it is not tested.  Same factor, fewer tests.
 * Works under the divergent control flow the shading code runs in (only shading lanes are active): the bounding box by LDS min / max on
 * order-preserving integer images of the coordinates, the (sphere, light) tests dealt over the ACTIVE lanes, the mask by LDS or.
 * s_cull: 8 words of LDS (6 box, 2 mask).  `part`: this lane traces at least one ray of the batch. */
__device__ __forceinline__ int wt_f2ord(float f) { const int b = __float_as_int(f); return b >= 0 ? b : (int)(0x80000000u - (unsigned)b); }
__device__ __forceinline__ float wt_ord2f(int o) { return __int_as_float(o >= 0 ? o : (int)(0x80000000u - (unsigned)o)); }
template <bool GEOM_LDS, int LCH>
__device__ __forceinline__ unsigned long long wt_sphere_candidates(const whitted_params& P, const float4* sg, unsigned g_lgt, unsigned lb, f3 ip,
                                                                   bool part, int* s_cull, unsigned lane) {
    const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
    const unsigned first = (unsigned)__builtin_ctzll(act);
    if (lane == first) {
        s_cull[0] = s_cull[1] = s_cull[2] = 0x7FFFFFFF; s_cull[3] = s_cull[4] = s_cull[5] = (int)0x80000000; s_cull[6] = s_cull[7] = 0;
    }
    if (part) {
        atomicMin(s_cull + 0, wt_f2ord(ip.x)); atomicMin(s_cull + 1, wt_f2ord(ip.y)); atomicMin(s_cull + 2, wt_f2ord(ip.z));
        atomicMax(s_cull + 3, wt_f2ord(ip.x)); atomicMax(s_cull + 4, wt_f2ord(ip.y)); atomicMax(s_cull + 5, wt_f2ord(ip.z));
    }
    const f3 lo = mk3(wt_ord2f(s_cull[0]), wt_ord2f(s_cull[1]), wt_ord2f(s_cull[2])), hi = mk3(wt_ord2f(s_cull[3]), wt_ord2f(s_cull[4]), wt_ord2f(s_cull[5]));
    const f3 m = (lo + hi) * 0.5f, hd = (hi - lo) * 0.5f;
    const float rho = sqrtf(dot3(hd, hd)) * 1.0001f;
    if (!(rho < 1e30f)) return ~0ull;                             /* a NaN or infinite shading point: everything is tested */
    const unsigned nact = (unsigned)__builtin_popcountll(act), rank = (unsigned)__builtin_popcountll(act & ((1ull << lane) - 1ull));
    for (unsigned i = rank; i < P.ns; i += nact) {                /* the spheres dealt over the active lanes */
        const float4 s = wt_geom<GEOM_LDS>(P, sg, i);             /* the UNMOVED centre, not wt_sphere_at: one mask serves every lane, so a launch with sphere motion must not call this (whitted_shade.inc asks !WT_MOTION.on first) */
        const f3 c = mk3(s.x, s.y, s.z);
        const float R = sqrtf(fabsf(s.w));
        bool near_ = false;
#pragma unroll
        for (int k = 0; k < LCH; k++) {
            if (lb + k < P.nl) {                                  /* wave-uniform */
                const float4 l0 = wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (lb + k));
                const float rl = fabsf(wt_geom<GEOM_LDS>(P, sg, g_lgt + 2 * (lb + k) + 1).w);
                const f3 ab = mk3(l0.x, l0.y, l0.z) - m, ac = c - m;
                const float ab2 = dot3(ab, ab);
                float tt = ab2 > 0.0f ? dot3(ac, ab) / ab2 : 0.0f;
                tt = fminf(fmaxf(tt, 0.0f), 1.0f);
                const f3 dv = ac - ab * tt;
                const float reach = (R + fmaxf(rho, rl)) * 1.001f + 1e-4f * (fabsf(c.x) + fabsf(c.y) + fabsf(c.z) + fabsf(m.x) + fabsf(m.y) + fabsf(m.z) + 1.0f);
                near_ |= !(dot3(dv, dv) > reach * reach);          /* (a NaN keeps the sphere) */
            }
        }
        if (near_) atomicOr((unsigned*)s_cull + 6 + (i >> 5), 1u << (i & 31u));
    }
    const unsigned long long mask = (unsigned long long)(unsigned)s_cull[6] | ((unsigned long long)(unsigned)s_cull[7] << 32);
    return mask;
}

/* testShadowPath (primitives.cl:396-442) for a BATCH of NR shadow rays that leave the same point `ip`: one
 * wave-uniform pass over the primitives tests all NR directions against each primitive (NR independent dependency
 * chains per lane, the origin-only half of every test computed once).  op[q] enters as 1 (ray to be traced) or 0 (no
 * ray) and leaves as the ray's shadow factor: an opaque sphere or any plane in front of the sample -> 0, each
 * transparent sphere in front -> x0.8.  The wave stops as soon as every ray of every live lane is decided. */
/* chunk / dlc: the batch is the NR / WT_SOFT lights of light chunk `chunk` (rays 2k, 2k+1 belong to light 3 chunk + k)
 * and dlc[k] = the distance from ip to that light's centre -- or chunk = ~0u when the rays are not tied to the
 * scene's lights (unit test).  With the light / plane side table (scene_prep.c) a plane's tests are then skipped for
 * the two rays of a light when NO lane of the wave can get "blocked" out of them: the shading point and the whole
 * light sphere lie on the same side of the plane, with margins ten times the rounding involved, so the reference's
 * predicate `b != 0 && 0 < num/b < tl` (primitives.cl:422-437) is false whatever the sample.  In render.map no plane
 * ever lies between a surface and a light: 12 of the 36 tests of a shaded hit go. */
template <bool GEOM_LDS, int NR, bool CULL, bool MASKED = false, int SHF = 0, bool SKIP = false>
__device__ __forceinline__ void wt_shadow_batch(const whitted_params& P, const float4* sg, unsigned g_pln, f3 ip,
                                                const f3 (&rd)[NR], const float (&tl)[NR], const float (&a4)[NR],
                                                const float (&a2)[NR], float (&op)[NR], unsigned chunk,
                                                const float (&dlc)[NR / WT_SOFT], const unsigned long long cand = ~0ull,
                                                const wt_motion mv = wt_motion{false, 0.0f, 0u}, const unsigned skip = 0u) {
    /* `skip` (SKIP: wt_trace_cull only; wave-uniform): bit k set = no ray of this batch, from any lane, can pass the line test of a sphere i
     * with i mod 4 = k (the bounce cull table, bounce_cull_host.h): the plain loop does not test those spheres. */
    /* `cand` (wave-uniform; scenes of <= 64 spheres): bit i clear = no ray of this batch, from any lane, can meet sphere i in front of its
     * sample (wt_sphere_candidates): the sphere is not tested.  Which spheres are tested never changes a factor: a skipped test could only fail. */
    typedef wt_shape<SHF> SH;                                /* SHF: the caller's FLAGS (compile-time counts, wt_shape) */
    const bool masked = MASKED && P.ns <= 64u;               /* (MASKED: deep builds; the other builds keep exactly the plain loop below) */
    unsigned long long todo = !masked ? 0ull : ((P.ns == 64u ? ~0ull : ((1ull << P.ns) - 1ull)) & cand);
    for (unsigned n = 0; todo != 0ull; n++) {
        const unsigned i = (unsigned)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        if ((n & 3u) == 3u) {   /* every fourth sphere: is any ray of any lane still undecided? */
            unsigned live = 0u;
#pragma unroll
            for (int q = 0; q < NR; q++) live |= __float_as_uint(op[q]);
            if (__builtin_amdgcn_ballot_w64(live != 0u) == 0) break;
        }
        const float4 s = wt_sphere_at<GEOM_LDS>(P, sg, i, mv);
        const sph_pre pre = wt_shadow_pre(ip, s);
        const float through = (__float_as_uint(s.w) >> 31) ? P.through : 0.0f;   /* x0.8 or blocked */
        float bq[NR], Dq[NR];
        bool any = false;
#pragma unroll
        for (int q = 0; q < NR; q++) any |= wt_shadow_disc_g<GEOM_LDS>(pre, rd[q], a4[q], bq[q], Dq[q]);
        if (__builtin_amdgcn_ballot_w64(any)) {                   /* somebody's line meets the sphere */
#pragma unroll
            for (int q = 0; q < NR; q++) {
                float t;
                bool hit = wt_shadow_root_g<GEOM_LDS>(bq[q], Dq[q], a2[q], t) && !(Dq[q] < 0);
                if (hit && !(t >= tl[q])) op[q] = op[q] * through;
            }
        }
    }
    for (unsigned i = 0; !masked && i < SH::ns(P); i++) {
        if ((i & 3u) == 3u) {   /* every fourth sphere: is any ray of any lane still undecided? */
            /* op >= 0: all six are zero iff the OR of their bit patterns is */
            unsigned live = 0u;
#pragma unroll
            for (int q = 0; q < NR; q++) live |= __float_as_uint(op[q]);
            if (__builtin_amdgcn_ballot_w64(live != 0u) == 0) break;
        }
        if (SKIP && ((skip >> (i & 3u)) & 1u)) continue;          /* wave-uniform */
        const float4 s = wt_sphere_at<GEOM_LDS>(P, sg, i, mv);
        const sph_pre pre = wt_shadow_pre(ip, s);
        const float through = (__float_as_uint(s.w) >> 31) ? P.through : 0.0f;   /* x0.8 or blocked */
        float bq[NR], Dq[NR];
        bool any = false;
#pragma unroll
        for (int q = 0; q < NR; q++) any |= wt_shadow_disc_g<GEOM_LDS>(pre, rd[q], a4[q], bq[q], Dq[q]);
        if (__builtin_amdgcn_ballot_w64(any)) {                   /* somebody's line meets the sphere */
#pragma unroll
            for (int q = 0; q < NR; q++) {
                float t;
                bool hit = wt_shadow_root_g<GEOM_LDS>(bq[q], Dq[q], a2[q], t) && !(Dq[q] < 0);
                if (hit && !(t >= tl[q])) op[q] = op[q] * through;
            }
        }
    }
    for (unsigned i = 0; i < SH::np(P); i++) {
        if ((i & 3u) == 0u) {   /* after the spheres, then every fourth plane */
            unsigned live = 0u;
#pragma unroll
            for (int q = 0; q < NR; q++) live |= __float_as_uint(op[q]);
            if (__builtin_amdgcn_ballot_w64(live != 0u) == 0) break;
        }
        const float4 n = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i);
        const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * i + 1);
        const float num = wt_plane_pre(ip, n, p0);
        bool skip[NR / WT_SOFT];
#pragma unroll
        for (int k = 0; k < NR / WT_SOFT; k++) skip[k] = false;
        if (CULL && SH::lpt(P) && chunk != ~0u) {                          /* wave-uniform */
            const float4 mu = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * SH::np(P) + 2 * SH::nl(P) + chunk * SH::np(P) + i);
            const float mus[3] = {mu.x, mu.y, mu.z};
            const float an = 1e-5f * fabsf(num) * mu.w;                    /* |num| in units of distance, x 1e-5 */
#pragma unroll
            for (int k = 0; k < NR / WT_SOFT && k < 3; k++) {
                /* same side (num = (p0 - ip).n has the sign opposite to the point's side) and clear of it */
                const bool cannot = (num * mus[k] < 0.0f) && (fabsf(mus[k]) > __builtin_fmaf(4e-6f, dlc[k], an));
                skip[k] = __builtin_amdgcn_ballot_w64(!cannot) == 0;
            }
        }
#pragma unroll
        for (int q = 0; q < NR; q++) {
            if (!skip[q / WT_SOFT]) {
                if (wt_plane_blocks(num, n, rd[q], tl[q])) op[q] = 0.0f;
            }
        }
    }
}

/* The prepared geometry stream of a small scene (whitted_params.h), staged in LDS once per workgroup */
/* (moving launches -- the WT_F_MOVE flavours -- stage the displacement table behind it: wt_sphere_at) */
template <bool MOVE = false>
__device__ __forceinline__ void wt_stage_scene(const whitted_params& P, float4* s_geom, unsigned tid, unsigned nthreads) {
    for (unsigned i = tid; i < P.geom_f4; i += nthreads) s_geom[i] = ((const float4*)P.geom)[i];
    if (MOVE) for (unsigned i = tid; i < P.ns; i += nthreads) s_geom[P.geom_f4 + i] = ((const float4*)P.ss_disp)[i];
    __syncthreads();
}

#include "whitted_terms.inc"

template <int FLAGS>
struct wt_cfg {
    static constexpr bool deep = (FLAGS & 2) != 0, occ = (FLAGS & 32) != 0, grid = (FLAGS & 16) != 0;
    static constexpr int lds_levels = deep ? (occ ? WT_LDS_LEVELS_DEEP_OCC : WT_LDS_LEVELS_DEEP) : WT_LDS_LEVELS;
    /* parents the DFS stack can hold: depth - 1 (a child is only pushed while sp + 1 < depth, whitted_bounce.inc) */
    static constexpr int max_levels = !deep ? 3 : ((FLAGS & 64) ? 7 : ((FLAGS & 128) ? 15 : CLW_MAX_DEPTH - 1));
    static constexpr int min_waves = deep ? (occ ? WT_OCC_WAVES : WT_MIN_WAVES) : ((grid && !WT_STRICT) ? WT_GRID_SHALLOW_WAVES : WT_SHALLOW_WAVES);
};
/* Sum (SUM) or maximum of `c` over the 64 lanes of a full wave, uniform in every lane: DPP row shifts fold each row of 16 into its lane 15,
 * two row broadcasts fold the four rows into lane 63, one v_readlane fetches it -- a handful of VALU instructions, where the __shfl_xor
 * butterfly is six ds_bpermute_b32 round trips through the LDS crossbar with a wait each.  Lanes a shift or broadcast does not reach
 * take 0, the identity of both operations on unsigned values; integer sums and maxima are exact in any order. */
template <bool SUM>
__device__ __forceinline__ unsigned wt_wave_reduce(unsigned c) {
#define WT_DPP_STEP(ctrl, rows) do { const unsigned t_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)c, ctrl, rows, 0xF, false); \
                                     c = SUM ? c + t_ : max(c, t_); } while (0)
    WT_DPP_STEP(0x111, 0xF);    /* row_shr:1 */
    WT_DPP_STEP(0x112, 0xF);    /* row_shr:2 */
    WT_DPP_STEP(0x114, 0xF);    /* row_shr:4 */
    WT_DPP_STEP(0x118, 0xF);    /* row_shr:8 */
    WT_DPP_STEP(0x142, 0xA);    /* row_bcast:15 into rows 1 and 3 */
    WT_DPP_STEP(0x143, 0xC);    /* row_bcast:31 into rows 2 and 3 */
#undef WT_DPP_STEP
    return (unsigned)__builtin_amdgcn_readlane((int)c, 63);
}

/* Supersampling resolve (whitted_params.h: ss_lg): the sum of `v` over the n x n lane group of this lane, n = 1 << lg, with the lanes of a
 * tile laid out x = lane & 7, y = lane >> 3 -- the butterfly xor 1, 2, 4 along x, then xor 8, 16, 32 along y, cut to lg steps per axis.
 * Every step is one plain fp32 add of the lane's value and its partner's, and a + b == b + a bit for bit, so all lanes of a group end with the
 * same bits (the order is part of the image's definition: x first, adjacent pairs).  All in registers: DPP inside a row of 16 lanes, the
 * gfx950 half-row / half-wave swaps across rows.  Call with the WHOLE wave active: a DPP read of a disabled lane does not return its value.
 *   xor 1, 2: quad_perm.  xor 4: row_half_mirror reads lane ^ 7, which sits in the quad of lane ^ 4 -- a quad is uniform after xor 1 and 2,
 *   and xor 4 only runs after both (n = 8).  xor 8: row_ror:8.  xor 16 / 32: v_permlane16_swap / v_permlane32_swap of two copies of the value
 *   leave (own, partner) in one order or the other depending on the lane's half; their sum is the same either way. */
__device__ __forceinline__ float wt_ss_resolve(float v, const unsigned lg) {
#define WT_SS_DPP(ctrl) v = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, false))
    WT_SS_DPP(0xB1);                    /* quad_perm:[1,0,3,2] */
    if (lg >= 2u) WT_SS_DPP(0x4E);      /* quad_perm:[2,3,0,1] */
    if (lg >= 3u) WT_SS_DPP(0x141);     /* row_half_mirror */
    WT_SS_DPP(0x128);                   /* row_ror:8 */
#undef WT_SS_DPP
    if (lg >= 2u) {
        const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(p[0]) + __uint_as_float(p[1]);
    }
    if (lg >= 3u) {
        const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(p[0]) + __uint_as_float(p[1]);
    }
    return v;
}

/* Progressive accumulation (whitted_params.h: acc_sum): the pixel's value of this frame -- r, g, b in [0, 1] -- joins its 12-byte record of
 * running sums, and the running mean comes back in its place.  scale = 1 / frames; 1.0f is the first frame, which stores without reading
 * (the buffer is never cleared).  One owner lane per output pixel and launch: plain loads and stores, no atomics; every operation rounds
 * once (the units are built without contraction), so a numpy fold of the constituent frames gives the same bits. */
__device__ __forceinline__ void wt_acc_fold(float* __restrict__ s, const float scale, float& r, float& g, float& b) {
    float sr = r, sg = g, sb = b;
    if (scale != 1.0f) { sr = s[0] + r; sg = s[1] + g; sb = s[2] + b; }
    s[0] = sr; s[1] = sg; s[2] = sb;
    r = fminf(sr * scale, 1.0f); g = fminf(sg * scale, 1.0f); b = fminf(sb * scale, 1.0f);
}

/* One tile (tiled launches) or one block of work-items: the whole trace of its pixels.  `wg` is the workgroup's number in
 * the launch's dispatch order (blockIdx.x). */
typedef const __attribute__((address_space(4))) whitted_params* wt_kparams_t;
/* the flavours that have a twin reading the primary-ray cull table (wt_trace_cull): shallow, 1 sample, rays generated in the kernel, linear scan */
constexpr bool wt_cull_flavour(int flags) { return (flags & (WT_F_DEEP | WT_F_GRID | WT_F_RAYS | WT_F_SS)) == 0; }
/* a tile's 16-bit entry of the table (whitted_params.h: whitted_kargs): the primary byte, and the bounce byte (bounce_cull_host.h) above it */
#define WT_CULLB_SHADOW_SHIFT 8u        /* bits 8-11: WT_BC_SHADOW << k */
#define WT_CULLB_REFL_SHIFT 12u         /* bits 12-13: WT_BC_REFL_SPHERES, WT_BC_REFL_LIGHTS, in the order of WT_CULL_SPHERES, WT_CULL_LIGHTS */
#define WT_CULLB_MASK 0x3F03u
static_assert(WT_BC_REFL_SPHERES << 8 == WT_CULL_SPHERES << WT_CULLB_REFL_SHIFT && WT_BC_REFL_LIGHTS << 8 == WT_CULL_LIGHTS << WT_CULLB_REFL_SHIFT &&
              WT_BC_EPS == WT_EPSILON, "the bounce byte as wt_trace_body reads it");
/* TABLE: the body of wt_trace_cull -- `Pk` then points at a whitted_kargs (the parameters first, the table's pointer behind them); false: the
 * body of wt_trace, `Pk` points at the whitted_params alone and nothing of the table is compiled */
template <int FLAGS, bool TABLE>
__device__ __forceinline__ void wt_trace_body(const wt_kparams_t Pk, const unsigned wg) {
    constexpr bool COUNT = (FLAGS & WT_F_COUNT) != 0;
    constexpr bool DEEP = (FLAGS & WT_F_DEEP) != 0;
    constexpr bool GEOM_LDS = (FLAGS & WT_F_GEOM_LDS) != 0;
    constexpr bool FROM_RAYS = (FLAGS & WT_F_RAYS) != 0;
    constexpr bool GRID = (FLAGS & WT_F_GRID) != 0;     /* spheres through the uniform grid (big scenes) */
    constexpr bool SS = (FLAGS & WT_F_SS) != 0;         /* supersampled launch: the epilogue resolves n x n samples per stored pixel */
    constexpr bool MOVE = SS && !GRID && (FLAGS & WT_F_MOVE) != 0;   /* moving spheres: every sphere read takes the lane's scene time */
    constexpr bool LIST = SS && (FLAGS & WT_F_LIST) != 0;            /* the refine pass of an adaptive launch: the tile list's length is on the device */
    constexpr bool SEEDED = !wt_acc_flagged(FLAGS) || (FLAGS & WT_F_ACC) != 0;   /* the kernel reads the seed offset ... */
    constexpr bool ACC = SEEDED && !FROM_RAYS;                                   /* ... and its epilogue carries the accumulation branch (fused launches only) */
    constexpr bool UNIT_CT = !WT_STRICT && GEOM_LDS && !FROM_RAYS && !GRID;   /* see whitted_hit.inc */
    /* The lights' visibility classes (wt_light_vis) are compiled into the STRICT build's small-scene kernels only: there the samples they
     * save cost an fp64 product and a libm sin / cos each (-13 % at C2).  Measured for the fast build, whose samples are two hardware
     * instructions: +4 % inside this batch loop, +19 % as a loop of its own with the remaining rays compacted over the wave -- the
     * six-ray batch traces a ray 3.6 times cheaper than any one-ray-per-lane scheme (profiles/r03_ab_experiments.txt). */
    constexpr bool CLASSES = WT_STRICT != 0 && GEOM_LDS && !GRID;
    /* The primary-ray cull table (whitted_params.h: whitted_kargs) is compiled into a TWIN of the shallow 1-sample kernels that generate their
     * rays and scan the spheres linearly (wt_trace_cull), which only launches with a table run; wt_trace itself, every flavour of it, is the
     * code it was (the deep kernels' split tiles start in the tail, not in this loop). */
    constexpr bool CULL = TABLE && wt_cull_flavour(FLAGS);
    static_assert(!TABLE || wt_cull_flavour(FLAGS), "no table twin of this flavour");

    constexpr int LDSL = wt_cfg<FLAGS>::lds_levels;
    __shared__ float s_stk[LDSL * WT_REC * WT_BLOCK];
    /* the tree-parallel tail's batch boundaries (deep builds; whitted_tpt.inc) */
    __shared__ unsigned short s_tpt_bs[(DEEP && !wt_cfg<FLAGS>::occ) ? WT_TPT_MAX_BATCHES + 2 : 1];
    __shared__ unsigned s_tpt_px[(DEEP && !wt_cfg<FLAGS>::occ) ? 3 * 64 : 1];          /* the tail's xorshift pass: state, first hit ordinal, hits of every pixel */
    /* the wave-level choice of candidate spheres for the shadow batch (wt_sphere_candidates) is compiled into the deep kernels of BIG launches (the
     * high-occupancy flavour: C3 -3 %) and of the strict build (C3 strict -12 %); in the low-occupancy flavour its registers cost render.map's
     * depth-15 launches 1-2 % */
    constexpr bool SPHCULL = DEEP && !GRID && (wt_cfg<FLAGS>::occ || WT_STRICT != 0);
    __shared__ int s_cull[SPHCULL ? 8 : 1];
    extern __shared__ float4 s_geom[];

    /* The launch parameters are read through the kernel-argument segment pointer: fields are loaded where they are used
     * instead of all ~100 words up front -- scalar spills 5 -> 0 (53 -> 0 in the grid build), vector spills 7 -> 2. */
    const whitted_params& P = *(const whitted_params*)Pk;
#if WT_TIMELINE
    const unsigned long long tl_entry = __builtin_amdgcn_s_memrealtime();   /* first instructions of the wave */
#endif
    /* list-driven launches are sized for the case that every tile is refined: a wave beyond the end of its XCD's list (most of them, in a
     * frame with flat regions) leaves before it stages anything -- one scalar load and a compare */
    if (LIST) { if ((wg >> 3) >= P.list_count[WT_LIST_COUNT_STRIDE * (wg & 7u)]) return; }

    /* ---- stage the prepared geometry in LDS ------------------------------------------------------------------- */
    if (GEOM_LDS) wt_stage_scene<MOVE>(P, s_geom, threadIdx.x, WT_BLOCK);
    const float4* sg = s_geom;
#if WT_TIMELINE
    const unsigned long long tl_staged = __builtin_amdgcn_s_memrealtime();
#endif
    WT_STAMP_DECL

    const unsigned tid = threadIdx.x;
    const unsigned lane = tid & 63u;

    /* ---- work-item -> pixel ------------------------------------------------------- */
    bool valid;
    unsigned item;          /* index into out / rays */
    unsigned x = 0, y = 0;  /* position inside this launch's row range (fused mode) */
    unsigned tile = 0xFFFFFFFFu;   /* row-major tile index (tiled mode) */
    unsigned part_lg = 0u, part = 0u; /* this wave serves part `part` of 2^part_lg of the tile */
    /* wave-uniform: the tile's entry of the cull table in the FIRST loop iteration -- bits 0-1 the groups of tests it skips (WT_CULL_*), bits 8-11
     * the sphere classes its shade's shadow batch skips --, in the second the two group bits again (from the entry's bits 12-13), then 0 */
    unsigned cullb = 0u;
    if (P.tiled) {
        /* workgroups are dealt to XCDs round-robin (b % 8): XCD k owns the tile rows r = 8m + k, so a
         * framebuffer line is written by one L2 and per-XCD work stays balanced.  Within an XCD's share
         * the tiles are served heaviest-first when the previous frame's costs are known (tile_order):
         * the expensive refraction tiles start early and the cheap ones fill the tail. */
        const unsigned tpr = (P.width + 7u) >> 3;            /* 8-px-wide tiles per row */
        const unsigned b = wg;
        unsigned trow, tcol;
        if (P.tile_order) {                                  /* packed: column | row << 12 | log2(parts) << 24 | part << 27; 0xFFFFFFFF = none */
            const unsigned t = P.tile_order[b];
            tcol = t & 0xFFFu; trow = (t >> 12) & 0xFFFu;
            part_lg = (t >> 24) & 7u; part = (t >> 27) & 15u;
            tile = (t == 0xFFFFFFFFu) ? t : trow * tpr + tcol;
        } else {
            const unsigned k = b & 7u, j = b >> 3;
            trow = (j / tpr) * 8u + k;
            tcol = j % tpr;
            tile = trow * tpr + tcol;
        }
        x = tcol * 8u + (lane & 7u);
        y = trow * 8u + (lane >> 3);
        /* a HEAVY tile of a deep launch is served by 2, 4, 8 or 16 wavefronts (wt_sched_build, from the previous frame's costs): part p of
         * 2^lg owns 64 >> lg of its pixels, the other lanes only help in the tree-parallel tail, which such a wave enters at once */
        valid = (tile != 0xFFFFFFFFu) && (x < P.width) && (y < P.rows) && ((lane >> (6u - part_lg)) == part);
        item = y * P.width + x;
        /* the tile's two bytes of the cull table: a scalar load of the word that holds them, issued here, first needed at the light probe */
        if (CULL) {
            typedef const __attribute__((address_space(1))) unsigned* wt_gwords_t;
            const uint8_t* tc = ((const __attribute__((address_space(4))) whitted_kargs*)Pk)->tile_cull;
            if (tc && tile != 0xFFFFFFFFu && trow * 8u < P.rows)      /* (the default order's grid is rounded up to 8 tile rows: those lie beyond the table) */
                cullb = (unsigned)__builtin_amdgcn_readfirstlane((int)((((wt_gwords_t)tc)[tile >> 1] >> ((tile & 1u) * 16u)) & WT_CULLB_MASK));
        }
    } else {
        item = wg * WT_BLOCK + tid;
        valid = item < P.n_items;
        if (P.band_stride > 1u) { y = item / P.width; x = item % P.width; }
    }
#if WT_TIMELINE
    asm volatile("" :: "v"(item), "v"(x), "v"(y));
    const unsigned long long tl_mapped = __builtin_amdgcn_s_memrealtime();
#endif
    /* global linear id: seeds the RNG and gives the pixel (id % W, id / W) */
    unsigned long long gid = P.id_offset + item;
    unsigned gy = y;                                            /* global row (tiled / banded mappings) */
    if (P.band_stride > 1u) {
        gy = ((y >> 3) * P.band_stride + P.band_phase) * 8u + (y & 7u);
        gid = (unsigned long long)gy * P.width + x;
    } else if (P.tiled) {
        gy = P.row_offset + y;                                  /* a tiled range starts on a row: id_offset = row_offset * W */
    }

    /* deeper DFS levels (depth > WT_LDS_LEVELS + 1): private scratch */
    constexpr int SCRL = wt_cfg<FLAGS>::max_levels - LDSL;                 /* levels kept in scratch */
    float deep[SCRL > 0 ? SCRL * WT_REC : 1];

    /* ---- primary ray (raygen.cl:13-24) or the ray buffer ---------------------------- */
    f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1), rgb = mk3(0, 0, 0);
    int depth = 0;
    if (valid) {
        if (FROM_RAYS) {
            const float4* rr = (const float4*)(P.rays + 16 * (size_t)item);
            float4 ro = rr[0], rd = rr[1], rc = rr[2];
            o = mk3(ro.x, ro.y, ro.z); d = mk3(rd.x, rd.y, rd.z); rgb = mk3(rc.x, rc.y, rc.z);
            depth = __float_as_int(rr[3].x);
        } else if (SS && P.ss_cams) {
            /* a table of sample cameras (wave-uniform branch, supersampled flavours only): the lane's sub-sample is fixed by its number --
             * ((lane & 7) mod n, (lane >> 3) mod n), the virtual row offset being a multiple of n -- so the shim lays the table out per lane:
             * 12 floats { im_corner, origin, up, right }, three coalesced 16-byte loads, once per wave */
            const float4* c = (const float4*)P.ss_cams + 3u * lane;
            const float4 c0 = c[0], c1 = c[1], c2 = c[2];
            d = wt_primary_dir_xy(mk3(c0.x, c0.y, c0.z), mk3(c2.y, c2.z, c2.w), mk3(c1.z, c1.w, c2.x), P.w_factor, P.h_factor, x, gy);
            o = mk3(c0.w, c1.x, c1.y);
        } else {
            if (P.tiled || P.band_stride > 1u) d = wt_primary_dir_xy(P.corner, P.right, P.up, P.w_factor, P.h_factor, x, gy);
            else d = wt_primary_dir(P.corner, P.right, P.up, P.w_factor, P.h_factor, (unsigned)gid, P.width);
            o = mk3(P.origin[0], P.origin[1], P.origin[2]);
        }
    }
    /* moving spheres (the WT_F_MOVE flavours: supersampled, and not the grid builds, whose cell lists are built for one set of centres):
     * the lane's sub-sample fixes its scene time, one coalesced load per wave */
    wt_motion mv = {false, 0.0f, 0u};
    if (MOVE) { mv.on = true; mv.t = P.ss_times[lane]; mv.off = P.geom_f4; }
    float n1 = WT_DEFAULT_N, f = 1.0f;
    int sp = 0;                         /* parents on the stack */
    unsigned rng = (unsigned)gid;       /* raytracing.cl:33: id 0 is the xorshift fixed point */
    if (SEEDED) rng += P.seed_offset;   /* (0 = the reference's seeds) */
    const int D = P.depth;
    bool active = valid && depth < D;

    unsigned c_seg = 0, c_shadow = 0, c_probe = 0, c_sky = 0, c_tex = 0, c_push = 0, c_iter = 0, c_witer = 0;
    unsigned c_traced = 0;              /* shadow rays really traced (c_shadow also counts the elided ones of zero-coefficient surfaces) */
    unsigned c_known = 0, c_visbad = 0; /* lights whose samples were decided by their visibility class; verification build: ... wrongly */
    unsigned c_tptrun = 0, c_tptfail = 0, c_tptnodes = 0;   /* tiles finished by the tree-parallel tail / that it gave up on; nodes it traced */

    /* the scene's counts (compile-time constants in the shaped flavour, wt_shape) and the offsets of planes and lights in the geometry */
    typedef wt_shape<FLAGS> SH;
    const unsigned g_pln = SH::ns(P), g_lgt = SH::ns(P) + 2 * SH::np(P);

    /* scheduling hint for the next frame's dispatch order.  Small scenes: per lane 1 per loop iteration, +3 when it shades;
     * the tile reports its most expensive pixel (the serial chain of a refraction tree is what makes a tile late).  Grid
     * builds (big scenes): how long the wave lived, in units of 256 shader cycles -- there a wave pays the longest walk of
     * its 64 lanes, walk by walk, which no per-pixel count sees: C4 3.19 -> 2.29 ms against the iteration count.
     * (Measured and dropped: the lifetime for every build -- C3 +5 %, it depends on what ran beside the wave -- and a
     * per-wave count of iterations, shade passes and walk rounds: worse than no sorting at all at C2.) */
    const unsigned long long t_begin = ((GRID || WT_COST_LIFETIME) && P.tile_cost) ? __builtin_amdgcn_s_memtime() : 0ull;
#if WT_TIMELINE
    const unsigned long long tl_begin = __builtin_amdgcn_s_memrealtime();
    unsigned long long tl_end = tl_begin;
#endif
    unsigned cost = 0;
#ifndef WT_LCH
#define WT_LCH 3                     /* lights shaded together: 3 x 2 samples = six shadow rays per batch */
#endif
    constexpr int LCH = WT_LCH, NR = LCH * WT_SOFT;

    /* The per-lane loop: every lane runs its own pixel, depth first; the six shadow rays of a hit are traced TOGETHER by their lane
     * (six independent chains, origin-only halves shared).
     * Deep builds (depth > 4) leave it once at most P.tpt_max lanes are alive: what is left of the tile -- the refraction trees of a
     * few pixels, a serial chain of up to hundreds of segments per pixel in this loop -- is then traced by the whole wave as one
     * pool of segments (whitted_tpt.inc, the tree-parallel tail).  Same arithmetic per ray and the same order of additions per pixel
     * either way: the image does not depend on where a segment ran.  Shallow launches are throughput-bound and do not carry the tail. */
    constexpr bool TPT = DEEP && !wt_cfg<FLAGS>::occ;      /* (the high-occupancy flavour is for throughput-bound launches and stays lean) */
    unsigned tpt_thresh = (TPT && P.tpt_cap != 0u) ? (part_lg != 0u ? 64u : P.tpt_max) : 0u;
    WT_STAMP(WT_ST_PROLOG);
    for (;;) {
    while ((unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(active)) > tpt_thresh) {
        if (active) {
            WT_STAMP(WT_ST_LOOP);
            bool ended = false, shade = false;
            /* set by the hit phase on every path that sets `shade`, read only under `shade`: left without
             * initialisers on purpose (in this per-lane loop they would cost a register move each per iteration) */
            f3 ip, nrm, view;
            mat_t m;
            float ks, kd;
            unsigned prim, texpx;      /* the primitive hit; its texel word when `textured` */
            bool textured;
#include "whitted_hit.inc"
            WT_STAMP(WT_ST_RESOLVE);
            if (shade) {
            /* ---- Phong + soft shadows (raytracing.cl:83-136) ---------------------
             * The 2 samples x 3 lights = 6 shadow rays of a hit leave from the same point, so they
             * are traced TOGETHER: the RNG stream is drawn first in the reference's order, then one
             * wave-uniform pass over the primitives tests all six directions against each primitive
             * (six independent dependency chains per lane instead of one, and the origin-only half
             * of every test is computed once).  testShadowPath (primitives.cl:396-442) per ray:
             * an opaque sphere or any plane in front of the sample -> 0, each transparent sphere
             * in front -> x0.8; `op` carries that product and is zeroed on the first blocker. */
            /* A surface whose specular and diffuse coefficients are both zero (glass) receives exactly
             * +0 from every light whatever the shadow term is, provided the factors it multiplies are
             * finite: its shadow rays are not traced (the RNG still advances).  Checked per light below. */
#include "whitted_shade.inc"
#include "whitted_bounce.inc"
            WT_STAMP(WT_ST_BOUNCE);
            }
#include "whitted_pop.inc"
            WT_STAMP(WT_ST_POP);
        }
        /* the table's low byte speaks of primary rays and of their shade: every live lane has just traced its own.  Its reflected bits move into
         * the two group bits for the second iteration (every live lane then traces the reflection off the tile's plane: bounce_cull_host.h), and
         * the same shift leaves 0 behind that one */
        if (CULL) cullb = (cullb >> WT_CULLB_REFL_SHIFT) & (WT_CULL_SPHERES | WT_CULL_LIGHTS);
    }
    if (!TPT || __builtin_amdgcn_ballot_w64(active) == 0) break;
    {
        bool tpt_done = false;
#include "whitted_tpt.inc"
        if (tpt_done) break;
        tpt_thresh = 0u;               /* the tail gave up (its arena is full): the rest runs in the per-lane loop */
    }
    }
    if (P.tiled && P.tile_cost) {       /* wave-uniform branch */
        unsigned c = cost;
        if (GRID || WT_COST_LIFETIME) c = (unsigned)min((__builtin_amdgcn_s_memtime() - t_begin) >> 8, 0xFFFFFFFFull);
        else if (P.untrimmed) {             /* variant 16384: the butterfly this reduction was before wt_wave_reduce */
            if (P.cost_sum) for (int off = 32; off > 0; off >>= 1) c += (unsigned)__shfl_xor((int)c, off);
            else for (int off = 32; off > 0; off >>= 1) c = max(c, (unsigned)__shfl_xor((int)c, off));
        }
        else if (P.cost_sum) c = wt_wave_reduce<true>(c);      /* the wave's total work */
        else c = wt_wave_reduce<false>(c);
#if WT_TIMELINE     /* DIAGNOSTIC: when in the launch did this wave run? (tools/timeline.py) */
        if (P.diag && P.diag < 256u) c = ((unsigned)((tl_begin >> (P.diag - 1u)) & 0xFFFFull) << 16) | (unsigned)((__builtin_amdgcn_s_memrealtime() >> (P.diag - 1u)) & 0xFFFFull);
        tl_end = __builtin_amdgcn_s_memrealtime();
#endif
        if (lane == 0 && tile != 0xFFFFFFFFu && y < P.rows) {
            if (P.cost_sum && !(WT_TIMELINE && P.diag)) atomicAdd(P.tile_cost + tile, c);     /* the parts of a tile add up (the shim zeroed the buffer) */
            else P.tile_cost[tile] = c;
        }
    }


    /* ---- supersampled launches: the n x n clamped samples of an output pixel are averaged across their lanes, one lane packs and stores.
     * n divides 8 and the virtual sizes are multiples of n, so a lane group is valid or invalid as a whole (a part of a split tile owns whole
     * tile rows, at least n of them: the shim caps the split); the cross-lane steps run with every lane active, only the store is predicated.
     * A flavour of its own (WT_F_SS), so that the 1-sample kernels are the code they were. */
    if (SS) {
        const unsigned lg = P.ss_lg, m = (1u << lg) - 1u;
        const float inv = __uint_as_float((127u - 2u * lg) << 23);      /* 1 / n^2, exact */
        const float mr = wt_ss_resolve(fminf(fmaxf(rgb.x, 0.0f), 1.0f), lg) * inv;
        const float mg = wt_ss_resolve(fminf(fmaxf(rgb.y, 0.0f), 1.0f), lg) * inv;
        const float mb = wt_ss_resolve(fminf(fmaxf(rgb.z, 0.0f), 1.0f), lg) * inv;
        if (valid && (lane & (m | (m << 3))) == 0u) {
            const size_t px = (size_t)(y >> lg) * (P.width >> lg) + (x >> lg);
            float vr = mr, vg = mg, vb = mb;
            if (ACC && P.acc_sum) wt_acc_fold(P.acc_sum + 3 * px, P.acc_scale, vr, vg, vb);      /* wave-uniform: the running mean of a still view */
            if (P.out_rgb) {
                float* q = P.out_rgb + 3 * px;
                q[0] = vr; q[1] = vg; q[2] = vb;
            }
            P.out[px] = ((unsigned)(vr * 255.0f) << 16) | ((unsigned)(vg * 255.0f) << 8) | (unsigned)(vb * 255.0f);
        }
    } else
    /* ---- pack (raytracing.cl:193-194): clamp, *255, truncate ---------------------------- */
    if (valid) {
        if (ACC && P.acc_sum) {      /* wave-uniform: the clamped sample joins the running sum, and the mean (in [0, 1]: the clamp below keeps it) takes its place */
            rgb = mk3(fminf(fmaxf(rgb.x, 0.0f), 1.0f), fminf(fmaxf(rgb.y, 0.0f), 1.0f), fminf(fmaxf(rgb.z, 0.0f), 1.0f));
            wt_acc_fold(P.acc_sum + 3 * (size_t)item, P.acc_scale, rgb.x, rgb.y, rgb.z);
        }
        if (P.out_rgb) {
            float* q = P.out_rgb + 3 * (size_t)item;
            q[0] = rgb.x; q[1] = rgb.y; q[2] = rgb.z;
        }
        float cr = fminf(fmaxf(rgb.x, 0.0f), 1.0f) * 255.0f;
        float cg = fminf(fmaxf(rgb.y, 0.0f), 1.0f) * 255.0f;
        float cb = fminf(fmaxf(rgb.z, 0.0f), 1.0f) * 255.0f;
        P.out[item] = ((unsigned)cr << 16) | ((unsigned)cg << 8) | (unsigned)cb;
    }

#ifdef WT_STAMPS
    WT_STAMP(WT_ST_LOOP);
    __syncthreads();
    if (P.counters && lane == 0) {   /* 1 024 shards behind the counter block: same-address atomics from 32 640 waves would
                                        congest the memory system the stamps are measuring */
        unsigned long long* sh = P.counters + CLW_NUM_COUNTERS + 16u * (wg & 1023u);
        for (int k = 0; k < WT_ST_N; k++) atomicAdd(sh + k, (unsigned long long)s_st[k]);
        atomicAdd(sh + WT_ST_N, 1ull);      /* waves */
    }
#endif
    if (COUNT) {
        unsigned v[14] = {c_seg, c_shadow, c_probe, c_sky, c_tex, c_push, c_iter, c_witer, c_traced, c_known, c_visbad, c_tptfail, c_tptrun, c_tptnodes};
#pragma unroll
        for (int k = 0; k < 14; k++) {
            unsigned x = v[k];
            for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
            if (lane == 0 && x) atomicAdd(P.counters + (k < 10 ? k : 18 + k), (unsigned long long)x);   /* words 0-9 and 28-31 */
        }
    }
#if WT_TIMELINE     /* diag >= 256: (prologue << 16 | epilogue) in 10 ns ticks -- entry to the first trace iteration, cost write to here */
    if (P.diag >= 256u && P.tiled && P.tile_cost && lane == 0 && tile != 0xFFFFFFFFu && y < P.rows) {
        __builtin_amdgcn_s_waitcnt(0);      /* the pixel stores have left */
        if (P.diag == 256u) P.tile_cost[tile] = ((unsigned)min(tl_begin - tl_entry, 0xFFFFull) << 16) | (unsigned)min(__builtin_amdgcn_s_memrealtime() - tl_end, 0xFFFFull);
        else P.tile_cost[tile] = ((unsigned)min(tl_staged - tl_entry, 1023ull) << 22) | ((unsigned)min(tl_mapped - tl_staged, 2047ull) << 11) | (unsigned)min(tl_begin - tl_mapped, 2047ull);
    }
#endif
}
/* The trace kernel: one workgroup (one wave) per tile. */
template <int FLAGS>
__global__ void __launch_bounds__(WT_BLOCK, wt_cfg<FLAGS>::min_waves) wt_trace(const whitted_params P_arg) {
    const wt_kparams_t Pk = (wt_kparams_t)__builtin_amdgcn_kernarg_segment_ptr();     /* = &P_arg */
    wt_trace_body<FLAGS, false>(Pk, blockIdx.x);
}
/* Its twin for a launch with a primary-ray cull table (the flavours of wt_cull_flavour only): the same body with the table's hooks compiled in.
 * The body reads the table's pointer THROUGH Pk, behind the parameters: that is whitted_kargs' layout, held here. */
static_assert(__builtin_offsetof(whitted_kargs, P) == 0 && __builtin_offsetof(whitted_kargs, tile_cull) == sizeof(whitted_params) && sizeof(whitted_params) % 8 == 0,
              "wt_trace_body<FLAGS, true> reads tile_cull behind the whitted_params its Pk points at");
template <int FLAGS>
__global__ void __launch_bounds__(WT_BLOCK, wt_cfg<FLAGS>::min_waves) wt_trace_cull(const whitted_kargs K_arg) {
    const wt_kparams_t Pk = (wt_kparams_t)__builtin_amdgcn_kernarg_segment_ptr();     /* = &K_arg.P */
    wt_trace_body<FLAGS, true>(Pk, blockIdx.x);
}

/* ---- the per-lane table of sample cameras (whitted_params.h: ss_cams) travels as a by-value kernel argument and is written by the launch
 *      stream itself: ordered behind the launches that read the previous table, no host memory to keep alive, no host wait. ---- */
__global__ void __launch_bounds__(64) wt_cams_store(const wt_cam_table T_arg, float4* __restrict__ dst) {
    typedef const __attribute__((address_space(4))) float4* kargs_t;
    const float4* src = (const float4*)(kargs_t)__builtin_amdgcn_kernarg_segment_ptr();   /* = &T_arg */
    (void)T_arg;
#pragma unroll
    for (unsigned k = 0; k < WT_CAM_TABLE_FLOATS / 4u / 64u; k++) dst[k * 64u + threadIdx.x] = src[k * 64u + threadIdx.x];
}

#define WT_RG_BLOCK 256
/* ---- standalone raygen (raygen.cl:5-25): the API-faithful, HBM-bound path.  Each lane
 *      builds its 64-B rray; records are transposed through LDS so every store
 *      instruction of a wave writes 1 KiB of contiguous memory. ------------------------ */
__global__ void __launch_bounds__(WT_RG_BLOCK) wt_raygen(const raygen_params P) {
    constexpr int RS = WT_RG_BLOCK + 1;            /* padded row: conflict-free both ways */
    __shared__ float4 s_rec[4 * RS];            /* [part][ray] */
    const unsigned tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * WT_RG_BLOCK;
    const size_t item = base + tid;
    float4 r0 = make_float4(0, 0, 0, 0), r1 = r0;
    if (item < P.n_items) {
        unsigned long long gid = P.id_offset + item;
        if (P.band_stride > 1u) {
            const unsigned y = (unsigned)(item / P.width), x = (unsigned)(item % P.width);
            gid = (unsigned long long)(((y >> 3) * P.band_stride + P.band_phase) * 8u + (y & 7u)) * P.width + x;
        }
        f3 d = wt_primary_dir(P.corner, P.right, P.up, P.w_factor, P.h_factor, (unsigned)gid, P.width);
        r0 = make_float4(P.origin[0], P.origin[1], P.origin[2], 0.0f);
        r1 = make_float4(d.x, d.y, d.z, 0.0f);
    }
    /* record = {origin, dir, rgb = 0, depth = 0 + pad}; rows 2,3 are zero */
    s_rec[0 * RS + tid] = r0;
    s_rec[1 * RS + tid] = r1;
    s_rec[2 * RS + tid] = make_float4(0, 0, 0, 0);
    s_rec[3 * RS + tid] = make_float4(0, 0, 0, 0);
    __syncthreads();
    float4* dst = (float4*)P.rays + base * 4;
    const size_t limit = ((size_t)P.n_items - base < WT_RG_BLOCK ? (size_t)P.n_items - base : WT_RG_BLOCK) * 4;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        size_t q = (size_t)k * WT_RG_BLOCK + tid;      /* float4 index inside the block's 16 KiB */
        if (q < limit) dst[q] = s_rec[(q & 3) * RS + (q >> 2)];
    }
}

/* ---- cost-sorted dispatch order: one workgroup per XCD share, counting sort (descending) of the
 *      previous frame's tile costs.  order[8*pos + k] = pos-th heaviest wavefront of XCD share k.
 *      Entry: tile column | tile row << 12 | log2(parts) << 24 | part << 27 (0xFFFFFFFF = none).
 *      split_slots != 0 (deep launches with the tree-parallel tail; costs are then a tile's TOTAL work): a tile whose cost exceeds the
 *      share's quota -- its total cost over the `split_slots` wavefronts the share's CUs hold at a time, at least `min_quota` -- is served
 *      by 2, 4, 8 or 16 wavefronts, each owning a part of its pixels and sorted in with cost / parts, so that what a launch waits for is its
 *      work, not its heaviest tile (800x600 depth 15: one tile's 560 us of the 570).  The share's list has `per_share_cap` entries; the
 *      quota doubles until the parts fit. ------------ */
__global__ void __launch_bounds__(256) wt_sched_build(const unsigned* __restrict__ cost, unsigned* __restrict__ order,
                                                      unsigned tpr, unsigned trows, unsigned per_share, unsigned clamp_outliers,
                                                      unsigned per_share_cap, unsigned split_slots, unsigned min_quota, unsigned max_lg) {
    __shared__ unsigned hist[256];
    __shared__ unsigned base[256];
    __shared__ unsigned s_max, s_cnt, s_entries;
    __shared__ unsigned long long s_sum;
    const unsigned k = blockIdx.x, tid = threadIdx.x;
    hist[tid] = 0;
    if (tid == 0) { s_max = 1u; s_cnt = 0u; s_sum = 0ull; s_entries = 0u; }
    __syncthreads();
    unsigned cnt = 0u;
    unsigned long long sum = 0ull;
    for (unsigned j = tid; j < per_share; j += 256) {
        const unsigned trow = (j / tpr) * 8u + k;
        if (trow < trows) { sum += cost[trow * tpr + (j % tpr)]; cnt++; }
    }
    atomicAdd(&s_sum, sum); atomicAdd(&s_cnt, cnt);
    __syncthreads();
    /* parts per tile: the smallest power of two that brings cost / parts under the quota, at most 2^max_lg (16; fewer in supersampled launches,
     * where a part must hold whole n x n sample groups: 8 >> lg tile rows >= n) */
    unsigned quota = 0xFFFFFFFFu;
    if (split_slots != 0u) {
        const unsigned long long q = s_sum / split_slots;
        quota = (unsigned)(q > 0x7FFFFFFFull ? 0x7FFFFFFFull : q);
        if (quota < min_quota) quota = min_quota;
        if (quota == 0u) quota = 1u;
        bool fitted = false;
        for (int trial = 0; trial < 24; trial++) {
            if (tid == 0) s_entries = 0u;
            __syncthreads();
            unsigned e = 0u;
            for (unsigned j = tid; j < per_share; j += 256) {
                const unsigned trow = (j / tpr) * 8u + k;
                if (trow < trows) { unsigned lg = 0u; const unsigned c = cost[trow * tpr + (j % tpr)]; while (lg < max_lg && (c >> lg) > quota) lg++; e += 1u << lg; }
            }
            atomicAdd(&s_entries, e);
            __syncthreads();
            const bool fits = s_entries <= per_share_cap;
            __syncthreads();
            if (fits) { fitted = true; break; }
            quota = quota > 0x3FFFFFFFu ? 0xFFFFFFFFu : quota * 2u;
        }
        /* the doubling reaches "never split" by itself only from a quota of 2^8 or more: a smaller one with huge costs gets there here, so
         * that the scatter below always stays inside the list (cnt <= per_share <= per_share_cap) */
        if (!fitted) quota = 0xFFFFFFFFu;
    }
    auto parts_lg = [&](unsigned c) { unsigned lg = 0u; while (lg < max_lg && (c >> lg) > quota) lg++; return lg; };
    /* costs are iteration counts, total work or wave durations (any range): 256 bins scaled by the share's maximum.  Durations have
     * outliers (a wave of a cold first frame can live a hundred times longer than the rest, which would squeeze every other
     * tile into bin 0 = no order at all): with `clamp_outliers` the scale stops at 16x the share's mean. */
    unsigned mx = 1u;
    for (unsigned j = tid; j < per_share; j += 256) {
        const unsigned trow = (j / tpr) * 8u + k;
        if (trow < trows) { const unsigned c = cost[trow * tpr + (j % tpr)]; mx = max(mx, c >> parts_lg(c)); }
    }
    atomicMax(&s_max, mx);
    __syncthreads();
    float top = (float)s_max;
    if (clamp_outliers && s_cnt != 0u) top = fminf(top, fmaxf(16.0f * (float)s_sum / (float)s_cnt, 1.0f));
    const float scale = top <= 255.0f ? 1.0f : 255.0f / top;   /* small costs keep one bin per value */
    for (unsigned j = tid; j < per_share; j += 256) {
        const unsigned trow = (j / tpr) * 8u + k;
        if (trow < trows) {
            const unsigned c0 = cost[trow * tpr + (j % tpr)], lg = parts_lg(c0);
            const unsigned c = (unsigned)fminf((float)(c0 >> lg) * scale, 255.0f);   /* (clamped as a float: with `clamp_outliers` the product can pass 2^32) */
            atomicAdd(&hist[255u - c], 1u << lg);
        }
    }
    __syncthreads();
    if (tid == 0) {
        unsigned acc = 0;
        for (int i = 0; i < 256; i++) { base[i] = acc; acc += hist[i]; }
        hist[0] = acc;                       /* number of wavefronts with a tile in this share */
    }
    __syncthreads();
    const unsigned nvalid = hist[0];
    for (unsigned j = tid; j < per_share; j += 256) {
        const unsigned trow = (j / tpr) * 8u + k;
        if (trow < trows) {
            const unsigned tcol = j % tpr, t = trow * tpr + tcol;
            const unsigned lg = parts_lg(cost[t]);
            const unsigned c = (unsigned)fminf((float)(cost[t] >> lg) * scale, 255.0f);
            const unsigned pos = atomicAdd(&base[255u - c], 1u << lg);
            for (unsigned q = 0; q < (1u << lg); q++) order[8u * (pos + q) + k] = tcol | (trow << 12) | (lg << 24) | (q << 27);
        }
    }
    for (unsigned j = nvalid + tid; j < per_share_cap; j += 256) order[8u * j + k] = 0xFFFFFFFFu;
}

/* ---- adaptive supersampling: the classifier between the 1-sample base pass and the list-driven refine pass (WT_F_LIST).
 *      frame = the packed base frame of the launch range, width x rows OUTPUT pixels.  A pixel is flagged when one of its R, G, B channels
 *      differs by at least `threshold` from the same channel of one of its 4-neighbours inside the range; a block of b x b pixels, b = 1 << lgb
 *      = 8 / n -- one 8x8 tile of the virtual frame -- is refined when any of its pixels is flagged (host definition: clw_host_refine_mask).
 *      A wave owns 64 / b^2 blocks of ONE block row, block g in the b^2 adjacent lanes g b^2 .. -- so a block's flag is a field of the
 *      wave's ballot, and all its blocks go to the same list: block (= virtual tile) row r belongs to XCD r mod 8, as in wt_sched_build, the
 *      eight lists interleaved as order[8 j + k].  One append per wave: the ballot of the refined blocks, one atomic add of its population
 *      count by the first of their lanes, the lanes' ranks from mbcnt.  mask[block] = 0 / 1 for every block; count[WT_LIST_COUNT_STRIDE * k]
 *      (zeroed by the shim) ends as the length of list k.  The order inside a list depends on which wave came first; mask and lengths do not.
 *      cap = entries per list: what every block of a share refined gives, so the guard below never fires. ------------ */
#if !WT_STRICT   /* integer work, the same in both arithmetic builds: compiled into the fast unit only (the shim launches that copy) */
__device__ __forceinline__ unsigned wt_px_contrast(unsigned p, unsigned q) {
    unsigned c = 0u;
#pragma unroll
    for (int s = 0; s < 24; s += 8) {
        const int d = (int)((p >> s) & 255u) - (int)((q >> s) & 255u);
        c = max(c, (unsigned)(d < 0 ? -d : d));
    }
    return c;
}
__global__ void __launch_bounds__(256) wt_refine_classify(const unsigned* __restrict__ frame, unsigned width, unsigned rows, unsigned lgb,
                                                          unsigned threshold, unsigned nbc, unsigned nbr, unsigned wpr,
                                                          unsigned char* __restrict__ mask, unsigned* __restrict__ order,
                                                          unsigned* __restrict__ count, unsigned cap) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (wave >= nbr * wpr) return;                                  /* wave-uniform */
    const unsigned br = wave / wpr, wc = wave % wpr;                /* the wave's block row, and which 64 / b^2 blocks of it */
    const unsigned b = 1u << lgb, sub = lane & (b * b - 1u);
    const unsigned bc = wc * (64u >> (2u * lgb)) + (lane >> (2u * lgb));
    const unsigned x = bc * b + (sub & (b - 1u)), y = br * b + (sub >> lgb);
    const bool in = x < width && y < rows;
    unsigned c = 0u;
    if (in) {                                                       /* the one-pixel halo, cut at the range's edges */
        const unsigned* p = frame + (size_t)y * width + x;
        const unsigned v = p[0];
        if (x > 0u) c = max(c, wt_px_contrast(v, p[-1]));
        if (x + 1u < width) c = max(c, wt_px_contrast(v, p[1]));
        if (y > 0u) c = max(c, wt_px_contrast(v, p[-(ptrdiff_t)width]));
        if (y + 1u < rows) c = max(c, wt_px_contrast(v, p[width]));
    }
    const unsigned long long flagged = __builtin_amdgcn_ballot_w64(in && c >= threshold);
    const bool lead = sub == 0u && in;                              /* a block's first pixel is inside the range iff the block is */
    const bool refined = lead && ((flagged >> lane) & ((1ull << (b * b)) - 1ull)) != 0ull;     /* b^2 <= 16 */
    if (lead) mask[(size_t)br * nbc + bc] = refined ? 1 : 0;
    const unsigned long long app = __builtin_amdgcn_ballot_w64(refined);
    if (app != 0ull) {
        const unsigned k = br & 7u, first = (unsigned)__builtin_ctzll(app);
        unsigned base = 0u;
        if (lane == first) base = atomicAdd(count + WT_LIST_COUNT_STRIDE * k, (unsigned)__builtin_popcountll(app));
        base = (unsigned)__builtin_amdgcn_readlane((int)base, (int)first);
        const unsigned j = base + __builtin_amdgcn_mbcnt_hi((unsigned)(app >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)app, 0u));
        if (refined && j < cap) order[8u * j + k] = bc | (br << 12);
    }
}
#endif

/* ---- unit-test kernel: the device helpers one by one, one input row per thread (tests/test_gpu_functions.py
 *      feeds it the golden vectors produced by the reference's own functions).  Rows are `stride_in` floats in,
 *      `stride_out` floats out. -------------------------------------------------------------------------------- */
enum { WT_U_SPHERE = 0, WT_U_PLANE = 1, WT_U_REFLECT = 2, WT_U_REFRACT = 3, WT_U_SCHLICK = 4, WT_U_CUBE = 5,
       WT_U_XORSHIFT = 6, WT_U_EMOD = 7, WT_U_SINCOS = 8, WT_U_POW = 9, WT_U_NORMALIZE = 10 };
__global__ void __launch_bounds__(64) wt_unit(int op, const float* __restrict__ in, float* __restrict__ out, unsigned n,
                                              unsigned stride_in, unsigned stride_out, unsigned aux) {
    const unsigned i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* a = in + (size_t)i * stride_in;
    float* r = out + (size_t)i * stride_out;
    switch (op) {
        case WT_U_SPHERE: {      /* o[3] d[3] c[3] radius -> hit, t */
            const rayq q = wt_rayq<false>(mk3(a[0], a[1], a[2]), mk3(a[3], a[4], a[5]));
            float t;
            bool hit = wt_sphere(q, make_float4(a[6], a[7], a[8], a[9] * a[9]), t);
            r[0] = hit ? 1.0f : 0.0f; r[1] = hit ? t : 0.0f;
        } break;
        case WT_U_PLANE: {       /* o[3] d[3] n[3] p0[3] -> hit, t */
            const rayq q = wt_rayq<false>(mk3(a[0], a[1], a[2]), mk3(a[3], a[4], a[5]));
            float t;
            bool hit = wt_plane(q, make_float4(a[6], a[7], a[8], 0.0f), make_float4(a[9], a[10], a[11], 0.0f), t);
            r[0] = hit ? 1.0f : 0.0f; r[1] = hit ? t : 0.0f;
        } break;
        case WT_U_REFLECT: {     /* i[3] n[3] -> r[3] */
            f3 v = wt_reflect(mk3(a[0], a[1], a[2]), mk3(a[3], a[4], a[5]));
            r[0] = v.x; r[1] = v.y; r[2] = v.z;
        } break;
        case WT_U_REFRACT: {     /* n1 n2 i[3] n[3] -> ok, r[3] */
            f3 v = mk3(0, 0, 0);
            bool ok = wt_refract(a[0], a[1], mk3(a[2], a[3], a[4]), mk3(a[5], a[6], a[7]), v);
            r[0] = ok ? 1.0f : 0.0f; r[1] = v.x; r[2] = v.y; r[3] = v.z;
        } break;
        case WT_U_SCHLICK:       /* n1 n2 i[3] n[3] -> fr */
            r[0] = wt_schlick(a[0], a[1], mk3(a[2], a[3], a[4]), mk3(a[5], a[6], a[7]));
            break;
        case WT_U_CUBE: {        /* dir[3] -> u, v (int bits); aux = face size */
            int u, v;
            wt_cube_uv(mk3(a[0], a[1], a[2]), aux, u, v);
            r[0] = __int_as_float(u); r[1] = __int_as_float(v);
        } break;
        case WT_U_XORSHIFT: {    /* state bits -> new state bits, value */
            unsigned st = __float_as_uint(a[0]);
            float v = wt_xorshift(st);
            r[0] = __uint_as_float(st); r[1] = v;
        } break;
        case WT_U_EMOD:          /* a, b (int bits) -> a mod b (int bits) */
            r[0] = __int_as_float(wt_emod(__float_as_int(a[0]), __float_as_int(a[1])));
            break;
        case WT_U_SINCOS: {      /* u -> sin, cos of fl32(2*pi*u) (aux = 1) or fl32(pi*u) (aux = 0) */
            float sn, cs;
            if (aux) wt_sincos_angle<true>(a[0], sn, cs); else wt_sincos_angle<false>(a[0], sn, cs);
            r[0] = sn; r[1] = cs;
        } break;
        case WT_U_POW:           /* x, y -> x^y */
            r[0] = wt_pow(a[0], a[1]);
            break;
        case WT_U_NORMALIZE: {   /* v[3] -> unit[3], length */
            float len;
            f3 v = wt_normalize_len(mk3(a[0], a[1], a[2]), len);
            r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = len;
        } break;
        default: break;
    }
}

/* ---- unit-test kernel for the helpers that need the SCENE: the kernel's own hit phase (whitted_hit.inc, textually the
 *      code wt_trace runs) and its batched shadow traversal, one input row per thread, against the golden vectors of the
 *      reference's findLightIntersection / findSolidIntersection / testShadowPath / plane_texture_pixel
 *      (primitives.cl:262-318, 322-394, 396-442, 217-259).
 *      WT_US_HIT    {o[3], d[3]} -> {lit, light rgb[3], solid hit, point[3], normal[3], material: rgb[3], ambient, diffuse,
 *                   specular, shininess, transparent, dielectric, n, reflectivity}                         (22 floats)
 *      WT_US_SHADOW {to[3], from[3]} -> {shadow factor}
 *      WT_US_TEXEL  {ptex row: b0[3], scale, b1[3], texture id bits; p[3]} -> {rgb[3]}   (rows 16-byte aligned) */
enum { WT_US_HIT = 0, WT_US_SHADOW = 1, WT_US_TEXEL = 2 };
template <bool GEOM_LDS, bool GRID>
__global__ void __launch_bounds__(64) wt_unit_scene(const whitted_params P, int op, const float* __restrict__ in,
                                                    float* __restrict__ out, unsigned n, unsigned stride_in, unsigned stride_out) {
    extern __shared__ float4 s_geom[];
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    constexpr bool UNIT_CT = false;                         /* the unit-test kernel takes rays as given */
    if (GEOM_LDS) wt_stage_scene(P, s_geom, tid, 64u);
    const float4* sg = s_geom;
    typedef wt_shape<0> SH;                               /* (the counts as whitted_hit.inc reads them: the launch's) */
    const unsigned g_pln = P.ns, g_lgt = P.ns + 2 * P.np;
    const unsigned i = blockIdx.x * 64 + tid;
    if (i >= n) return;
    const float* a = in + (size_t)i * stride_in;
    float* res = out + (size_t)i * stride_out;
    WT_STAMP_DECL
    constexpr bool COUNT = false, FROM_RAYS = false;    /* like the fused kernel: the test rows carry unit directions */
    constexpr bool CULL = false; constexpr unsigned cullb = 0u;      /* any ray, not a tile's primary rays: every test runs */
    unsigned cost = 0, c_iter = 0, c_witer = 0, c_probe = 0, c_seg = 0, c_sky = 0, c_tex = 0;
    const wt_motion mv = {false, 0.0f, 0u};             /* the unit-test kernel sees the scene as it stands */
    (void)lane; (void)c_iter; (void)c_witer; (void)c_probe; (void)c_seg; (void)c_sky; (void)c_tex;
    if (op == WT_US_HIT) {
        f3 o = mk3(a[0], a[1], a[2]), d = mk3(a[3], a[4], a[5]), rgb = mk3(0, 0, 0);
        const float f = 1.0f;
        bool ended = false, shade = false;
        f3 ip = mk3(0, 0, 0), nrm = mk3(0, 0, 0), view = mk3(0, 0, 0);
        mat_t m;
        m.rgb = mk3(0, 0, 0); m.ambient = m.diffuse = m.specular = m.shininess = 0.0f;
        m.transparent = m.dielectric = 0u; m.n = 0.0f; m.reflectivity = 0.0f;
        float ks = 0.0f, kd = 0.0f;
        unsigned prim = 0u, texpx = 0u;
        bool textured = false;
        {
#include "whitted_hit.inc"
            res[0] = lit ? 1.0f : 0.0f;
            if (lit) { res[1] = rgb.x; res[2] = rgb.y; res[3] = rgb.z; }      /* f = 1, rgb = 0 on entry: the light's colour */
        }
        (void)ended; (void)view; (void)ks; (void)kd; (void)cost;
        res[4] = shade ? 1.0f : 0.0f;
        if (shade) {
            if (textured) m.rgb = wt_texel_rgb(texpx);
            res[5] = ip.x; res[6] = ip.y; res[7] = ip.z; res[8] = nrm.x; res[9] = nrm.y; res[10] = nrm.z;
            res[11] = m.rgb.x; res[12] = m.rgb.y; res[13] = m.rgb.z; res[14] = m.ambient; res[15] = m.diffuse; res[16] = m.specular;
            res[17] = m.shininess; res[18] = (float)m.transparent; res[19] = (float)m.dielectric; res[20] = m.n; res[21] = m.reflectivity;
        }
    } else if (op == WT_US_SHADOW) {
        const f3 to = mk3(a[0], a[1], a[2]), from = mk3(a[3], a[4], a[5]);
        constexpr int NR = WT_SOFT * 3;
        f3 rd[NR]; float tl[NR], a4[NR], a2[NR], opq[NR];
#pragma unroll
        for (int q = 0; q < NR; q++) { rd[q] = mk3(0, 0, 0); tl[q] = 0.0f; a4[q] = 0.0f; a2[q] = 0.0f; opq[q] = 0.0f; }
        rd[0] = wt_normalize_len(to - from, tl[0]);
        const rayq rq = wt_shadow_rayq_scene<GEOM_LDS>(P, from, rd[0]);
        a4[0] = rq.a4; a2[0] = rq.a2; opq[0] = 1.0f;
        if (GRID) {
            opq[0] = wt_grid_shadow(P, from, rd[0], rq.a4, rq.a2, tl[0]);
            for (unsigned k = 0; k < P.np; k++) {
                const float4 pn = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * k);
                const float4 p0 = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * k + 1);
                if (wt_plane_blocks(wt_plane_pre(from, pn, p0), pn, rd[0], tl[0])) opq[0] = 0.0f;
            }
        } else {
            const float dlc[NR / WT_SOFT] = {0.0f, 0.0f, 0.0f};
            wt_shadow_batch<GEOM_LDS, NR, false>(P, sg, g_pln, from, rd, tl, a4, a2, opq, ~0u, dlc);
        }
        res[0] = opq[0];
    } else if (op == WT_US_TEXEL) {
        whitted_params Q = P;
        Q.ptex = a;                                              /* this row's basis / scale / texture id */
        const f3 c = wt_texel_rgb(wt_plane_texel_fetch(Q, 0u, mk3(a[8], a[9], a[10])));
        res[0] = c.x; res[1] = c.y; res[2] = c.z;
    }
}
