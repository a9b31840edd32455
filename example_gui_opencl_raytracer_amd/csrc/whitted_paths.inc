/* whitted_paths.inc -- path queries (hip_wrap_ext.h: clw_ext_cast_paths, clw_ext_cast_paths_device, clw_ext_pick_path): where a caller's ray
 * GOES -- its hit, the reference's reflected or refracted ray from there, that ray's hit, and so on for up to 8 segments -- in one launch.
 * Included by whitted_launch.inc behind whitted_layers.inc, so it exists in the fast and the strict unit.  csrc/paths_host.c is the definition.
 * A segment is wt_cast's nearest query: the one scan of whitted_query.inc (wt_query_scan: the flat scan and the grid walk, their arithmetic and
 * its proof) with wt_cast's sink (wt_sink_nearest), and wt_cast's evaluation of the winner.  No trace kernel and no other pass is touched.
 *
 * Mapping: wt_cast's -- one ray per lane, one wave per workgroup (one batch of 64 rays), the scene staged by wt_stage_scene, read from global
 * memory, or walked through the uniform grid.  The lane's path lives in registers: the current ray, the refractive index n1, the count and the
 * reason.  The loop runs over segments and is wave-uniform: a lane whose path has ended runs along and tests nothing (`live` is the scan's
 * `valid`), and the wave leaves the loop when none of its lanes is live.  The number of segments is a run-time argument: the loop body is one
 * scan, a compile-time count would unroll nothing worth having.
 * The winner's four material words -- transperent, dielectric, n, reflectivity -- are read from the bound sphere / plane array itself
 * (wt_mat_f4: one 16-byte load at byte 64 of the 96-byte record, for the winner only, as the trace kernels gather materials), not from a
 * prepared table: a table would be one more thing to build and to invalidate with the scene, to spare one load per SEGMENT beside a scan
 * that makes one per primitive.
 * Output: hits[seg * n + ray] (2 float4 per clw_hit), layer-major; the layers a path does not reach receive the miss record.  status[ray] =
 * count | reason << 4.  next (may be null): the ray the path would go on with, see the header. */

struct wt_paths_args {
    const float4* rays;         /* 2 per ray: {origin, tmax}, {dir, bits(ignore)} */
    float4* hits;               /* 2 per ray and segment: {t, bits(id), normal.xy}, {normal.z, point}; segment-major */
    unsigned char* status;      /* 1 per ray */
    float4* next;               /* 2 per ray, or null */
    unsigned n, flags, bounces;
};

#define WT_PATH_TRANSMIT 16u
#define WT_PATH_ALL_SURFACES 32u
#define WT_PATH_EPSILON 0.001f      /* primitives.cl:5 */
#define WT_PATH_DEFAULT_N 1.0f      /* raytracing.cl:7 */

/* primitives.cl:127-130, the definition's operations (paths_host.c: reflect) */
__device__ __forceinline__ f3 wt_path_reflect(f3 i, f3 n) {
#pragma clang fp contract(off)
    const float k = 2 * -wt_gb_ref_dot(n, i);
    return mk3(i.x + n.x * k, i.y + n.y * k, i.z + n.z * k);
}

/* primitives.cl:132-144 (paths_host.c: refract): false = total internal reflection (the reference's NaN vector) */
__device__ __forceinline__ bool wt_path_refract(float n1, float n2, f3 i, f3 nrm, f3& out) {
#pragma clang fp contract(off)
    const float n = n1 / n2;
    const float cosI = -wt_gb_ref_dot(nrm, i);
    const float sinT2 = n * n * (1.0f - cosI * cosI);
    if (sinT2 > 1.0f) return false;
    const float w = n * cosI - sqrtf(1.0f - sinT2);
    out = mk3(i.x * n + nrm.x * w, i.y * n + nrm.y * w, i.z * n + nrm.z * w);
    return !(out.x != out.x);      /* (a NaN x from NaN terms counts as the reference's NaN vector does) */
}

__device__ __forceinline__ void wt_path_store_hit(float4* hits, size_t at, float t, unsigned id, f3 nrm, f3 ip) {
    hits[2 * at] = make_float4(t, __uint_as_float(id), nrm.x, nrm.y);
    hits[2 * at + 1] = make_float4(nrm.z, ip.x, ip.y, ip.z);
}

template <bool GEOM_LDS, bool GRID>
__global__ void __launch_bounds__(WT_BLOCK) wt_cast_paths(const whitted_params P, const wt_paths_args A) {
    extern __shared__ float4 s_geom[];
    if (GEOM_LDS) wt_stage_scene(P, s_geom, threadIdx.x, WT_BLOCK);
    const float4* sg = s_geom;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned g_pln = P.ns, g_lgt = P.ns + 2 * P.np;

    const unsigned base = blockIdx.x * 64u;      /* (the launcher keeps groups * 64 below 2^31) */
    if (base >= A.n) return;
    const bool valid = base + lane < A.n;
    const unsigned k = valid ? base + lane : A.n - 1u;      /* (a lane past the end reads the last ray, tests nothing and stores nothing) */
    wt_query_ray r = wt_query_load(A.rays, k);
    const unsigned cast_flags = A.flags & (WT_CAST_SPHERES | WT_CAST_PLANES | WT_CAST_LIGHTS | WT_CAST_OPAQUE);
    float n1 = WT_PATH_DEFAULT_N;
    unsigned count = 0u, reason = 0u;
    bool live = valid;

    unsigned seg = 0u;
    for (; seg < A.bounces; seg++) {      /* (wave-uniform) */
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;      /* every path of the wave has ended */
        wt_sink_nearest B;
        wt_query_scan<GEOM_LDS, GRID>(P, sg, r, cast_flags, live, B);
        if (!live) {      /* an ended path's layer: the miss record */
            if (valid) wt_path_store_hit(A.hits, (size_t)seg * A.n + k, INFINITY, WT_GB_ID_NONE, mk3(0, 0, 0), mk3(0, 0, 0));
            continue;
        }
        if (B.id == WT_GB_ID_NONE) {      /* a miss: r stays the ray that missed */
            wt_path_store_hit(A.hits, (size_t)seg * A.n + k, B.t, WT_GB_ID_NONE, mk3(0, 0, 0), mk3(0, 0, 0));
            reason = 1u; live = false;
            continue;
        }
        /* the winner's point and normal, as wt_cast evaluates them */
        const unsigned kind = B.id >> 30, index = B.id & 0x3FFFFFFFu;
        const f3 ip = wt_gb_ref_madd(r.d, B.t, r.o);
        f3 nrm;
        if (kind == 1u) {
            const float4 pn = wt_geom<GEOM_LDS>(P, sg, g_pln + 2 * index);
            nrm = mk3(pn.x, pn.y, pn.z);      /* never flipped toward the ray */
        } else {
            const float4 s = wt_geom<GEOM_LDS>(P, sg, kind == 0u ? index : g_lgt + 2 * index);
            nrm = wt_gb_ref_normalize(ip - mk3(s.x, s.y, s.z));
        }
        wt_path_store_hit(A.hits, (size_t)seg * A.n + k, B.t, B.id, nrm, ip);
        count = seg + 1u;

        const f3 p = wt_gb_ref_madd(nrm, WT_PATH_EPSILON, ip);      /* the point shading uses */
        bool stops = kind == 2u;      /* a light */
        float4 m = make_float4(0, 0, 0, 0);      /* bits(transperent), bits(dielectric), n, reflectivity */
        if (!stops) {
            m = wt_mat_f4(P, kind == 0u ? index : P.ns + index, 2u, P.ns);
            stops = !(A.flags & WT_PATH_ALL_SURFACES) && m.w == 0 && __float_as_uint(m.y) == 0u && __float_as_uint(m.x) == 0u;
        }
        if (stops) {
            r.o = p; r.d = mk3(0, 0, 0); r.ignore = WT_GB_ID_NONE;
            reason = 2u; live = false;
            continue;
        }
        /* the outgoing ray (paths_host.c: bounce) */
        f3 o = p, d = wt_path_reflect(r.d, nrm);
        if ((A.flags & WT_PATH_TRANSMIT) && __float_as_uint(m.x) != 0u) {
#pragma clang fp contract(off)
            const float n2 = (n1 == WT_PATH_DEFAULT_N) ? m.z : WT_PATH_DEFAULT_N;
            const bool entering = n1 < n2;
            const float e2 = 2 * WT_PATH_EPSILON;
            const f3 inside = mk3(p.x - nrm.x * e2, p.y - nrm.y * e2, p.z - nrm.z * e2);
            const f3 face = entering ? nrm : mk3(nrm.x * -1.0f, nrm.y * -1.0f, nrm.z * -1.0f);
            f3 through;
            if (wt_path_refract(n1, n2, r.d, face, through)) {
                o = entering ? inside : p;
                d = through;
                n1 = n2;
            }
        }
        r.o = o; r.d = d; r.ignore = WT_GB_ID_NONE;
        r.a = wt_gb_ref_dot(d, d);
    }
    if (!valid) return;
    for (; seg < A.bounces; seg++)      /* the layers no path of the wave reached */
        wt_path_store_hit(A.hits, (size_t)seg * A.n + k, INFINITY, WT_GB_ID_NONE, mk3(0, 0, 0), mk3(0, 0, 0));
    A.status[k] = (unsigned char)(count | reason << 4);
    if (A.next) {
        A.next[2 * (size_t)k] = make_float4(r.o.x, r.o.y, r.o.z, r.tmax);
        A.next[2 * (size_t)k + 1] = make_float4(r.d.x, r.d.y, r.d.z, __uint_as_float(r.ignore));
    }
}
